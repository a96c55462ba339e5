// Stand-alone check of the multi-scan host stage (csrc/jpeg_multiscan.h) on hostile input, meant to be built with
// -fsanitize=address,undefined and run on the CPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vision-transformers-pytorch_amd/csrc \
//       tools/jpeg_multiscan_check.cpp -o jpeg_multiscan_check && ./jpeg_multiscan_check file.jpg [more.jpg ...]
//
// Per file (progressive, multi-scan sequential or single-scan): the whole decode, a few windows, the file truncated at EVERY
// length, and a single-byte corruption at every position (one XOR pattern per position, three patterns in turn).  Every call must
// return -- success or a defined reason code -- with every read inside the file and every write inside the buffers it was given:
// file, coefficients and scratch are heap blocks of exactly the advertised sizes, so the sanitizer sees one byte too many.  A
// decode that succeeds must have written a plan record jpeg_plan_valid accepts.  Exit status 0 when nothing was flagged.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "jpeg_multiscan.h"

static int runs = 0, ok = 0;
static int reasons[32];

static void decode(const std::vector<unsigned char>& d, const int* window) {
  std::vector<unsigned char> exact(d);                      // a heap copy of exactly len bytes: an over-read is flagged
  VtxJpegInfo info;
  ++runs;
  int rc = jpeg_info_ex(exact.data(), exact.size(), &info, 1);
  if (rc < 0 || rc > 17 || rc != info.reason) { fprintf(stderr, "undefined reason %d\n", rc); exit(2); }
  if (rc) { ++reasons[rc]; return; }
  const size_t need = jpeg_coef_bytes_of(&info, window), nscratch = jpeg_scratch_bytes_of(&info);
  if (need == 0) { ++reasons[VTX_JPEG_WINDOW]; return; }
  if (info.reserved[0] != VTX_JPEG_KIND_SINGLE && nscratch == 0) { ++reasons[VTX_JPEG_TOO_LARGE]; return; }
  std::vector<unsigned char> coef(need), scratch(nscratch);
  VtxJpegPlan plan;
  const long long offs[3] = {0, 0, 0};
  rc = jpeg_entropy_decode_ms(exact.data(), exact.size(), window, coef.data(), coef.size(), offs, &plan,
                              nscratch ? scratch.data() : nullptr, nscratch);
  if (rc < 0 || rc > 17) { fprintf(stderr, "undefined reason %d\n", rc); exit(2); }
  ++reasons[rc];
  if (rc == 0) {
    ++ok;
    if (!jpeg_plan_valid(plan, need, need / 2, (size_t)plan.rows * plan.cols * 3)) { fprintf(stderr, "valid decode, invalid plan\n"); exit(2); }
  } else {
    const unsigned char* p = (const unsigned char*)&plan;
    for (size_t i = 0; i < sizeof(plan); ++i) if (p[i]) { fprintf(stderr, "failed decode, record not zeroed\n"); exit(2); }
  }
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s file.jpg [...]\n", argv[0]); return 2; }
  int kinds[3] = {0, 0, 0};
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { perror(argv[a]); return 2; }
    std::vector<unsigned char> d;
    unsigned char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + n);
    fclose(f);
    VtxJpegInfo info;
    if (jpeg_info_ex(d.data(), d.size(), &info, 1) != 0) { fprintf(stderr, "%s: refused, reason %d\n", argv[a], info.reason); return 2; }
    ++kinds[info.reserved[0]];
    const int H = info.height, W = info.width, before = ok;
    decode(d, nullptr);
    const int wins[5][4] = {{0, 0, 1, 1}, {H - 1, W - 1, 1, 1}, {H / 2, W / 3, H - H / 2, W - W / 3}, {0, 0, H, W}, {0, 0, H + 1, W}};
    for (const auto& w : wins) decode(d, w);
    if (ok - before != 5) { fprintf(stderr, "%s: the intact file did not decode (%d of 5)\n", argv[a], ok - before); return 2; }
    for (size_t k = 0; k < d.size(); ++k) decode(std::vector<unsigned char>(d.begin(), d.begin() + k), nullptr);
    static const unsigned char pat[3] = {0x01, 0x5A, 0xFF};
    for (size_t k = 0; k < d.size(); ++k) {
      std::vector<unsigned char> c(d);
      c[k] ^= pat[k % 3];
      decode(c, k % 5 == 0 ? wins[2] : nullptr);
    }
  }
  printf("%d files (%d single-scan, %d multi-scan sequential, %d progressive): %d decodes, %d succeeded; by reason:", argc - 1, kinds[0],
         kinds[1], kinds[2], runs, ok);
  for (int r = 0; r < 32; ++r) if (reasons[r]) printf(" %d:%d", r, reasons[r]);
  printf("\n");
  return 0;
}
