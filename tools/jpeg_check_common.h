// What the three stand-alone JPEG check programs share (tools/jpeg_host_check.cpp, jpeg_sync_check.cpp, jpeg_multiscan_check.cpp):
// the file reader, the mutation loops, the by-reason counts and the digest of the summary line.  Each program defines
//
//   static void decode(const std::vector<unsigned char>& d, const int* window);
//
// which runs its stage once, counts the outcome with jc_count and feeds the digest, and hands it to jc_main.
//
// Per file: the whole decode, five windows, the file truncated at EVERY length, and a single-byte corruption at every position
// (one XOR pattern per position, three patterns in turn; every fifth position decodes a window).  The digest is a 64-bit FNV-1a
// over every call's return code, its header record and, on success, every record and buffer the call wrote: two builds of one
// program whose digests are equal answered every call alike.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "jpeg_multiscan.h"

static int jc_runs = 0, jc_ok = 0;
static int jc_reasons[32];
static uint64_t jc_hash = 0xcbf29ce484222325ull;

static inline void jc_digest(const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) jc_hash = (jc_hash ^ b[i]) * 0x100000001b3ull;
}

// the outcome of one call: its reason, counted and digested (a reason outside the table ends the run)
static inline void jc_count(int reason) {
  if (reason < 0 || reason > 17) { fprintf(stderr, "undefined reason %d (run %d)\n", reason, jc_runs); exit(2); }
  ++jc_reasons[reason];
  if (reason == 0) ++jc_ok;
  const int32_t r = reason;
  jc_digest(&r, sizeof(r));
}

static inline bool jc_read(const char* path, std::vector<unsigned char>* d) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return false; }
  unsigned char buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) d->insert(d->end(), buf, buf + n);
  fclose(f);
  return true;
}

// the intact file of H x W pixels (when `accepted`, it and four of its five windows must decode), then its mutations
template <class Decode>
static inline bool jc_file(const char* path, const std::vector<unsigned char>& d, int H, int W, bool accepted, Decode decode) {
  const int before = jc_ok;
  decode(d, nullptr);
  const int wins[5][4] = {{0, 0, 1, 1}, {H - 1, W - 1, 1, 1}, {H / 2, W / 3, H - H / 2, W - W / 3}, {0, 0, H, W}, {0, 0, H + 1, W}};
  for (const auto& w : wins) decode(d, w);
  if (accepted && jc_ok - before != 5) { fprintf(stderr, "%s: the intact file did not decode (%d of 5)\n", path, jc_ok - before); return false; }
  for (size_t k = 0; k < d.size(); ++k) decode(std::vector<unsigned char>(d.begin(), d.begin() + k), nullptr);
  static const unsigned char pat[3] = {0x01, 0x5A, 0xFF};
  for (size_t k = 0; k < d.size(); ++k) {
    std::vector<unsigned char> c(d);
    c[k] ^= pat[k % 3];
    decode(c, k % 5 == 0 ? wins[2] : nullptr);
  }
  return true;
}

// main: every file named must be accepted with bit 0 of `flags` (vtx_jpeg_info_ex's) set; a file that flags 0 refuses (a progressive
// or multi-scan one) still goes through the loops, where every call must refuse it.  Then the summary line.
template <class Decode>
static inline int jc_main(int argc, char** argv, int flags, Decode decode) {
  if (argc < 2) { fprintf(stderr, "usage: %s file.jpg [...]\n", argv[0]); return 2; }
  int kinds[3] = {0, 0, 0};
  for (int a = 1; a < argc; ++a) {
    std::vector<unsigned char> d;
    if (!jc_read(argv[a], &d)) return 2;
    VtxJpegInfo info;
    if (jpeg_info_ex(d.data(), d.size(), &info, 1) != 0) { fprintf(stderr, "%s: refused, reason %d\n", argv[a], info.reason); return 2; }
    ++kinds[info.reserved[0]];
    if (!jc_file(argv[a], d, info.height, info.width, (flags & 1) || info.reserved[0] == VTX_JPEG_KIND_SINGLE, decode)) return 2;
  }
  printf("%d files (%d single-scan, %d multi-scan sequential, %d progressive): %d decodes, %d succeeded, digest %016llx; by reason:", argc - 1,
         kinds[0], kinds[1], kinds[2], jc_runs, jc_ok, (unsigned long long)jc_hash);
  for (int r = 0; r < 32; ++r) if (jc_reasons[r]) printf(" %d:%d", r, jc_reasons[r]);
  printf("\n");
  return 0;
}
