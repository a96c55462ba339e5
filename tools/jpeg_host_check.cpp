// Stand-alone check of the host entropy stage (csrc/jpeg_host.h) on hostile input, meant to be built with
// -fsanitize=address,undefined and run on the CPU:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vision-transformers-pytorch_amd/csrc \
//       tools/jpeg_host_check.cpp -o jpeg_host_check && ./jpeg_host_check file.jpg [more.jpg ...]
//
// Files, windows and mutations: tools/jpeg_check_common.h.  Every call must return -- success or a reason code -- with every
// write inside the buffer it was given (the buffer is allocated at exactly the advertised size, so the sanitizer sees one byte
// too many).  Exit status 0 when nothing was flagged.
#include "jpeg_check_common.h"

static void decode(const std::vector<unsigned char>& d, const int* window) {
  std::vector<unsigned char> exact(d);                      // a heap copy of exactly len bytes: an over-read is flagged
  VtxJpegInfo info;
  ++jc_runs;
  const int refused = jpeg_info_ex(exact.data(), exact.size(), &info, 0);
  jc_digest(&info, sizeof(info));
  if (refused != info.reason) { fprintf(stderr, "return code %d, reason %d\n", refused, info.reason); exit(2); }
  if (refused) { jc_count(refused); return; }
  const size_t need = jpeg_coef_bytes_of(&info, window);
  if (need == 0) { jc_count(VTX_JPEG_WINDOW); return; }
  std::vector<unsigned char> coef(need);
  VtxJpegPlan plan;
  const long long offs[3] = {0, 0, 0};
  const int rc = jpeg_entropy_decode(exact.data(), exact.size(), window, coef.data(), coef.size(), offs, &plan);
  jc_count(rc);
  if (rc == 0) {
    if (!jpeg_plan_valid(plan, need, need / 2, (size_t)plan.rows * plan.cols * 3)) { fprintf(stderr, "valid decode, invalid plan\n"); exit(2); }
    jc_digest(&plan, sizeof(plan));
    jc_digest(coef.data(), need);
  }
}

int main(int argc, char** argv) { return jc_main(argc, argv, 0, decode); }
