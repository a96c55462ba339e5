// Host check of the merge of the lists of a sharded bank: drives knn_merge_place_lists of csrc/knn_select.h -- the lines
// knn_merge_lists_kernel of csrc/knn.hip runs -- against a sort-based answer.  Stand-alone (own main, no GPU, never loaded
// into Python):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vision-transformers-pytorch_amd/csrc \
//       tools/knn_merge_check.cpp -o knn_merge_check && ./knn_merge_check
//
// A bank of n scores is cut into nlist consecutive shards of random sizes (empty ones included); every shard's list is the
// first min(k, rows of the shard) pairs of a stable descending sort of its scores, with shard-LOCAL indices, stored at
// list_stride apart in arrays allocated to EXACTLY the last real pair (so that the sanitizer sees any read of a place at or
// beyond lens[t]); the gaps between lists hold a poison that would win every comparison.  knn_merge_place_lists must put
// exactly the first k pairs of the whole bank -- higher score first, among equal scores the lower GLOBAL index first -- at
// places 0 .. k - 1, each once, and give every other pair a place >= k.  Exit code 0 and "knn_merge_check: N cases ok"
// when everything agrees.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "knn_select.h"

namespace {

struct Pair { float v; int32_t g; };

int g_cases = 0, g_failed = 0;
uint32_t g_rng = 2463534242u;
uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

void fail(const char* what, int n, int k, int nlist, int extra) {
  std::fprintf(stderr, "FAIL %s: n = %d, k = %d, nlist = %d, %d\n", what, n, k, nlist, extra);
  ++g_failed;
}

std::vector<float> scores(int n, int kind) {
  std::vector<float> s(n);
  for (int j = 0; j < n; ++j) {
    switch (kind) {
      case 0: s[j] = 1.f; break;                                                 // every score ties: the index alone decides
      case 1: s[j] = (float)(rnd() % 5) * 0.125f; break;                         // five distinct scores: heavy ties
      case 2: s[j] = (float)(rnd() % 100000) * 1e-3f - 50.f; break;              // hardly any tie
      case 3: s[j] = (float)j; break;                                            // the last shard holds the answer
      default: s[j] = (j % 7 == 3) ? std::numeric_limits<float>::quiet_NaN()
                      : (j % 5 == 1 ? -std::numeric_limits<float>::infinity() : (float)(rnd() % 3)); break;
    }
  }
  return s;
}

// first rows of the nlist shards that n rows are cut into.  style 0: even; 1: random cuts (ragged, some empty); 2: cuts
// drawn from {0, n / 3, 2 n / 3, n} (most shards empty, the first and the last ones among them)
std::vector<int32_t> cut(int n, int nlist, int style) {
  std::vector<int32_t> bases(nlist, 0);
  for (int t = 1; t < nlist; ++t) {
    if (style == 0) bases[t] = (int32_t)((int64_t)n * t / nlist);
    else if (style == 1) bases[t] = (int32_t)(rnd() % (uint32_t)(n + 1));
    else bases[t] = (int32_t)((int64_t)n * (rnd() % 4) / 3);
  }
  std::sort(bases.begin() + 1, bases.end());
  return bases;
}

void check(int n, int k, int nlist, int kind, int style) {
  ++g_cases;
  const std::vector<float> raw = scores(n, kind);
  const std::vector<int32_t> bases = cut(n, nlist, style);
  std::vector<int32_t> lens(nlist);
  const int64_t stride = k + (int64_t)(rnd() % 3);                               // list_stride >= k
  std::vector<std::vector<Pair>> lists(nlist);
  int64_t last = 0;                                                              // one past the last real pair
  for (int t = 0; t < nlist; ++t) {
    const int b = bases[t], e = t + 1 < nlist ? bases[t + 1] : n;
    std::vector<Pair> sh;
    for (int j = b; j < e; ++j) sh.push_back(Pair{raw[j], (int32_t)(j - b)});      // local index, NaN kept as it is
    std::stable_sort(sh.begin(), sh.end(), [](const Pair& a, const Pair& c) { return knn_clean(a.v) > knn_clean(c.v); });
    if ((int)sh.size() > k) sh.resize(k);
    lens[t] = (int32_t)sh.size();
    lists[t] = sh;
    if (lens[t] > 0) last = t * stride + lens[t];
  }
  std::vector<float> val((size_t)last, std::numeric_limits<float>::infinity());  // poison between the lists
  std::vector<int32_t> idx((size_t)last, -1);
  for (int t = 0; t < nlist; ++t)
    for (int p = 0; p < lens[t]; ++p) { val[(size_t)(t * stride + p)] = lists[t][p].v; idx[(size_t)(t * stride + p)] = lists[t][p].g; }

  std::vector<Pair> want(n);
  for (int j = 0; j < n; ++j) want[j] = Pair{knn_clean(raw[j]), (int32_t)j};
  std::stable_sort(want.begin(), want.end(), [](const Pair& a, const Pair& c) { return a.v > c.v; });
  const int kk = std::min(k, n);

  std::vector<int> seen(kk, 0);
  for (int s = 0; s < nlist; ++s)
    for (int p = 0; p < lens[s]; ++p) {
      const int place = knn_merge_place_lists(val.data(), idx.data(), lens.data(), bases.data(), nlist, stride, s, p);
      const float v = knn_clean(lists[s][p].v);
      const int32_t g = bases[s] + lists[s][p].g;
      if (place < 0) { fail("negative place", n, k, nlist, place); return; }
      if (place >= kk) {                                                         // not in the answer: must not be one of the first k
        for (int w = 0; w < kk; ++w) if (want[w].g == g) { fail("left out", n, k, nlist, w); return; }
        continue;
      }
      if (!(v == want[place].v) || g != want[place].g) { fail("wrong pair", n, k, nlist, place); return; }
      ++seen[place];
    }
  for (int p = 0; p < kk; ++p)
    if (seen[p] != 1) { fail("place not taken once", n, k, nlist, p); return; }
}

}  // namespace

int main() {
  const int ks[] = {1, 2, 5, 20, 64, 65, 200, 256};
  const int nls[] = {1, 2, 3, 8, 37, 64};
  for (int k : ks)
    for (int nlist : nls) {
      const int ns[] = {k, k + 1, 3 * k + 2, 1000};
      for (int n : ns)
        for (int kind = 0; kind <= 4; ++kind)
          for (int style = 0; style <= 2; ++style) check(n, k, nlist, kind, style);
    }
  // fewer rows than k: every pair has its place, the places 0 .. n - 1 are taken once
  for (int n : {1, 7, 19})
    for (int nlist : {1, 4, 64})
      for (int kind = 0; kind <= 4; ++kind) check(n, 20, nlist, kind, 1);
  if (g_failed) { std::fprintf(stderr, "knn_merge_check: %d of %d cases FAILED\n", g_failed, g_cases); return 1; }
  std::printf("knn_merge_check: %d cases ok\n", g_cases);
  return 0;
}
