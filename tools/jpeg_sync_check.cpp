// Stand-alone check of the self-synchronising entropy decoder (csrc/jpeg_sync.h: the code the device kernel runs, here with the
// lanes as a sequential loop) on hostile input, meant to be built with -fsanitize=address,undefined and run on the CPU:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vision-transformers-pytorch_amd/csrc \
//       tools/jpeg_sync_check.cpp -o jpeg_sync_check && ./jpeg_sync_check file.jpg [more.jpg ...]
//
// Per file: the whole decode, a few windows, then the file truncated at each of 20 evenly spaced lengths and with each of 50
// seeded single-byte corruptions of its entropy-coded segment (and 50 of its headers).  Every buffer is allocated at exactly the
// advertised size, so the sanitizer sees one byte too many.  Each result is compared with the host stage (csrc/jpeg_host.h):
// refused by one exactly when refused by the other, and equal coefficient bytes and plan records where both accept.  Exit
// status 0 when nothing was flagged and nothing differed.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "jpeg_sync.h"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (unsigned)(rng_state >> 32);
}

static int runs = 0, ok = 0, max_rounds = 0, not_converged = 0;
static int reasons[16];

static void fail(const char* what) { fprintf(stderr, "MISMATCH: %s (run %d)\n", what, runs); exit(3); }

static void decode(const std::vector<unsigned char>& d, const int* window) {
  std::vector<unsigned char> exact(d);                      // a heap copy of exactly len bytes: an over-read is flagged
  JpegHeader hdr;
  ++runs;
  if (jpeg_parse_header(exact.data(), exact.size(), &hdr) != 0) { ++reasons[hdr.info.reason & 15]; return; }
  const size_t need = jpeg_coef_bytes_of(&hdr.info, window);
  if (need == 0) { ++reasons[VTX_JPEG_WINDOW]; return; }
  std::vector<unsigned char> ref(need), coef(need, 7);
  VtxJpegPlan rplan, plan;
  const long long offs3[3] = {0, 0, 0};
  const int want = jpeg_entropy_decode(exact.data(), exact.size(), window, ref.data(), ref.size(), offs3, &rplan);

  const size_t sb = js_stream_bytes_of(exact.data(), exact.size()), gb = js_segment_bytes_of(&hdr.info);
  const size_t nsub = js_subsequences_of(&hdr.info, sb);
  if (!sb || !gb || !nsub) fail("size query refused an accepted header");
  std::vector<unsigned char> stream(sb), segs(gb);
  std::vector<JsScan> scan(1);
  const long long offs[6] = {0, 0, 0, 0, 0, 0};
  int got = js_prepare(exact.data(), exact.size(), window, offs, stream.data(), stream.size(), segs.data(), segs.size(), scan.data(), &plan);
  if (got == 0) {
    if ((size_t)scan[0].nsub > nsub || (size_t)scan[0].stream_bytes > sb) fail("prepare wrote more than the size queries said");
    const size_t wsb = js_workspace_bytes_of(1, gb, (size_t)scan[0].nsub);
    std::vector<uint32_t> ws(wsb / 4);
    if (!js_scan_valid(scan[0], segs.data(), sb, gb, need, (size_t)scan[0].nsub)) fail("prepare wrote a record the check refuses");
    uint32_t* arrays = ws.data() + (js_ws_scans(1) + js_align(gb, 256)) / 4;
    const JsCtx x = js_context(&scan[0], scan[0].dc, scan[0].ac, stream.data(), segs.data(), coef.data(), arrays, (size_t)scan[0].nsub);
    int rounds = 0;
    got = js_emulate_image(x, JS_ROUND_CAP, &rounds);
    if (rounds > max_rounds) max_rounds = rounds;
    if (got == VTX_JPEG_NOT_CONVERGED) {                     // the fallback: legitimate, but counted
      ++not_converged;
      got = want;
      coef = ref; plan = rplan;
    }
  }
  if (got != want) { fprintf(stderr, "host stage %d, emulation %d\n", want, got); fail("status"); }
  ++reasons[got & 15];
  if (got == 0) {
    ++ok;
    if (memcmp(coef.data(), ref.data(), need) != 0) fail("coefficients");
    if (memcmp(&plan, &rplan, sizeof(plan)) != 0) fail("plan record");
  }
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s file.jpg [...]\n", argv[0]); return 2; }
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { perror(argv[a]); return 2; }
    std::vector<unsigned char> d;
    unsigned char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + n);
    fclose(f);
    JpegHeader hdr;
    if (jpeg_parse_header(d.data(), d.size(), &hdr) != 0) { fprintf(stderr, "%s: refused, reason %d\n", argv[a], hdr.info.reason); return 2; }
    const int H = hdr.info.height, W = hdr.info.width;
    decode(d, nullptr);
    const int wins[5][4] = {{0, 0, 1, 1}, {H - 1, W - 1, 1, 1}, {H / 2, W / 3, H - H / 2, W - W / 3}, {0, 0, H, W}, {0, 0, H + 1, W}};
    for (const auto& w : wins) decode(d, w);
    for (int k = 0; k < 20; ++k) decode(std::vector<unsigned char>(d.begin(), d.begin() + d.size() * k / 20), nullptr);
    for (int k = 0; k < 100; ++k) {
      std::vector<unsigned char> c(d);
      const size_t lo = k < 50 ? hdr.scan_pos : 2, hi = k < 50 ? d.size() : hdr.scan_pos;
      c[lo + rnd() % (hi - lo)] = (unsigned char)rnd();
      decode(c, k % 3 == 0 ? wins[2] : nullptr);
    }
  }
  printf("%d decodes, %d succeeded, most rounds %d, not converged %d; by reason:", runs, ok, max_rounds, not_converged);
  for (int r = 0; r < 16; ++r) if (reasons[r]) printf(" %d:%d", r, reasons[r]);
  printf("\n");
  return 0;
}
