// Stand-alone check of the self-synchronising entropy decoder (csrc/jpeg_sync.h: the code the device kernel runs, here with the
// lanes as a sequential loop) on hostile input, meant to be built with -fsanitize=address,undefined and run on the CPU:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vision-transformers-pytorch_amd/csrc \
//       tools/jpeg_sync_check.cpp -o jpeg_sync_check && ./jpeg_sync_check file.jpg [more.jpg ...]
//
// Files, windows and mutations: tools/jpeg_check_common.h.  Every buffer is allocated at exactly the advertised size, so the
// sanitizer sees one byte too many.  Each result is compared with the host stage (csrc/jpeg_host.h): refused by one exactly when
// refused by the other, and equal coefficient bytes and plan records where both accept.  Exit status 0 when nothing was flagged
// and nothing differed.
#include <string.h>

#include "jpeg_check_common.h"
#include "jpeg_sync.h"

static int max_rounds = 0, not_converged = 0;

static void fail(const char* what) { fprintf(stderr, "MISMATCH: %s (run %d)\n", what, jc_runs); exit(3); }

static void decode(const std::vector<unsigned char>& d, const int* window) {
  std::vector<unsigned char> exact(d);                      // a heap copy of exactly len bytes: an over-read is flagged
  VtxJpegInfo info;
  ++jc_runs;
  const int refused = jpeg_info_ex(exact.data(), exact.size(), &info, 0);
  jc_digest(&info, sizeof(info));
  if (refused) { jc_count(refused); return; }
  const size_t need = jpeg_coef_bytes_of(&info, window);
  if (need == 0) { jc_count(VTX_JPEG_WINDOW); return; }
  std::vector<unsigned char> ref(need), coef(need, 7);
  VtxJpegPlan rplan, plan;
  const long long offs3[3] = {0, 0, 0};
  const int want = jpeg_entropy_decode(exact.data(), exact.size(), window, ref.data(), ref.size(), offs3, &rplan);

  const size_t sb = js_stream_bytes_of(exact.data(), exact.size()), gb = js_segment_bytes_of(&info);
  const size_t nsub = js_subsequences_of(&info, sb);
  if (!sb || !gb || !nsub) fail("size query refused an accepted header");
  std::vector<unsigned char> stream(sb), segs(gb);
  std::vector<JsScan> scan(1);
  const long long offs[6] = {0, 0, 0, 0, 0, 0};
  int got = js_prepare(exact.data(), exact.size(), window, offs, stream.data(), stream.size(), segs.data(), segs.size(), scan.data(), &plan);
  const int32_t prepared = got;
  jc_digest(&prepared, sizeof(prepared));
  if (got == 0) {
    if ((size_t)scan[0].nsub > nsub || (size_t)scan[0].stream_bytes > sb) fail("prepare wrote more than the size queries said");
    jc_digest(&plan, sizeof(plan));
    jc_digest(&scan[0], sizeof(JsScan));
    jc_digest(segs.data(), (size_t)scan[0].nseg * sizeof(JsSeg));
    jc_digest(stream.data(), (size_t)scan[0].stream_bytes);
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
  jc_count(got);
  if (got == 0) {
    if (memcmp(coef.data(), ref.data(), need) != 0) fail("coefficients");
    if (memcmp(&plan, &rplan, sizeof(plan)) != 0) fail("plan record");
    jc_digest(coef.data(), need);
  }
}

int main(int argc, char** argv) {
  const int rc = jc_main(argc, argv, 0, decode);
  printf("most rounds %d, not converged %d\n", max_rounds, not_converged);
  return rc;
}
