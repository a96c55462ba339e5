// Host check of the k-NN selection rule: drives csrc/knn_select.h -- the lines the kernels of csrc/knn.hip run -- against a
// sort-based answer.  Stand-alone (own main, no GPU, never loaded into Python):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vision-transformers-pytorch_amd/csrc \
//       tools/knn_select_check.cpp -o knn_select_check && ./knn_select_check
//
// Streams: a k-list that starts as k sentinels receives n pairs in arrival order through knn_enters + knn_insert_place (every
// place computed from the unchanged list, then all written -- what a wave does); the result must be the first min(n, k)
// pairs of a std::stable_sort by descending score, the rest sentinels.  Merges: the stream is cut into 1, 2 or 7 consecutive
// slabs, each with its own list; knn_merge_place must put exactly the first k pairs of the whole stream at places 0 .. k - 1,
// each once.  Exit code 0 and "knn_select_check: N cases ok" when everything agrees.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <utility>
#include <vector>

#include "knn_select.h"

namespace {

struct Pair { float v; int32_t i; };

int g_cases = 0, g_failed = 0;

void fail(const char* what, int n, int k, int extra) {
  std::fprintf(stderr, "FAIL %s: n = %d, k = %d, %d\n", what, n, k, extra);
  ++g_failed;
}

// the k-list of `stream` (pairs in arrival order) by the header's insert
void run_list(const std::vector<Pair>& stream, int k, std::vector<float>& val, std::vector<int32_t>& idx) {
  val.assign(k, knn_neg_inf());
  idx.assign(k, KNN_NO_INDEX);
  std::vector<float> nv(k);
  std::vector<int32_t> ni(k);
  for (const Pair& c : stream) {
    const float cv = knn_clean(c.v);
    if (!knn_enters(cv, c.i, val.data(), idx.data(), k)) continue;
    for (int p = 0; p < k; ++p) knn_insert_place(val.data(), idx.data(), p, cv, c.i, &nv[p], &ni[p]);
    val = nv;
    idx = ni;
  }
}

// sort-based answer: stable descending sort of the scores (pairs arrive in ascending index within what is sorted)
std::vector<Pair> answer(std::vector<Pair> all, int k) {
  std::sort(all.begin(), all.end(), [](const Pair& a, const Pair& b) { return a.i < b.i; });
  std::stable_sort(all.begin(), all.end(), [](const Pair& a, const Pair& b) { return a.v > b.v; });
  if ((int)all.size() > k) all.resize(k);
  return all;
}

void check_stream(const char* what, const std::vector<Pair>& stream, int k) {
  ++g_cases;
  const int n = (int)stream.size();
  std::vector<float> val;
  std::vector<int32_t> idx;
  run_list(stream, k, val, idx);
  const std::vector<Pair> want = answer(stream, k);
  for (int p = 0; p < k; ++p) {
    const bool real = p < (int)want.size();
    const float wv = real ? want[p].v : knn_neg_inf();
    const int32_t wi = real ? want[p].i : KNN_NO_INDEX;
    if (!(val[p] == wv) || idx[p] != wi) { fail(what, n, k, p); return; }
  }
}

void check_merge(const char* what, const std::vector<Pair>& stream, int k, int nlist) {
  ++g_cases;
  const int n = (int)stream.size();
  const int per = (n + nlist - 1) / nlist;
  std::vector<float> val((size_t)nlist * k);
  std::vector<int32_t> idx((size_t)nlist * k);
  for (int s = 0; s < nlist; ++s) {
    const int b = std::min(n, s * per), e = std::min(n, (s + 1) * per);
    std::vector<Pair> slab(stream.begin() + b, stream.begin() + e);          // may be empty: a list of sentinels
    std::vector<float> v;
    std::vector<int32_t> ix;
    run_list(slab, k, v, ix);
    std::copy(v.begin(), v.end(), val.begin() + (size_t)s * k);
    std::copy(ix.begin(), ix.end(), idx.begin() + (size_t)s * k);
  }
  const std::vector<Pair> want = answer(stream, k);
  std::vector<int> seen(k, 0);
  for (int s = 0; s < nlist; ++s)
    for (int p = 0; p < k; ++p) {
      const int place = knn_merge_place(val.data(), idx.data(), nlist, k, s, p);
      if (place >= k) continue;
      if (place < 0 || place >= (int)want.size() || !(val[(size_t)s * k + p] == want[place].v) ||
          idx[(size_t)s * k + p] != want[place].i) { fail(what, n, k, place); return; }
      ++seen[place];
    }
  for (int p = 0; p < (int)want.size(); ++p)
    if (seen[p] != 1) { fail(what, n, k, -p - 1); return; }
}

uint32_t g_rng = 12345u;
uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

std::vector<Pair> make(int n, int kind, int k) {
  std::vector<Pair> s(n);
  for (int j = 0; j < n; ++j) {
    float v;
    switch (kind) {
      case 0: v = 1.f; break;                                            // all scores equal
      case 1: v = (float)j; break;                                       // strictly ascending arrival
      case 2: v = (float)(n - j); break;                                 // strictly descending arrival
      case 3: v = (float)(rnd() % 7) * 0.125f; break;                    // few distinct scores: ties everywhere
      case 4: v = j < k / 2 ? 2.f : 1.f; break;                          // duplicated scores across the k-th place
      case 5: v = (float)(rnd() % 100000) * 1e-3f - 50.f; break;         // random, hardly any tie
      default: v = (j % 11 == 3) ? std::numeric_limits<float>::quiet_NaN()
                   : (j % 13 == 5 ? -std::numeric_limits<float>::infinity() : (float)(rnd() % 50)); break;   // NaN and -inf
    }
    s[j] = Pair{v, (int32_t)j};
  }
  return s;
}

}  // namespace

int main() {
  const int ks[] = {1, 2, 5, 20, 64, 65, 200, 256};
  for (int k : ks) {
    const int ns[] = {1, k - 1, k, k + 1, 2 * k + 3, 7 * k + 1, 1000};           // shorter than, equal to, longer than k
    for (int n : ns) {
      if (n < 1) continue;
      for (int kind = 0; kind <= 6; ++kind) {
        std::vector<Pair> s = make(n, kind, k);
        if (kind == 6) {                                                         // the answer orders NaN as -inf too
          std::vector<Pair> c = s;
          for (Pair& p : c) p.v = knn_clean(p.v);
          check_stream("stream (non-finite)", c, k);
          continue;
        }
        check_stream("stream", s, k);
        if (n >= k)
          for (int nlist : {1, 2, 7}) check_merge("merge", s, k, nlist);
      }
    }
  }
  // arrival in descending index (the insert does not rely on ascending arrival)
  for (int k : {3, 20, 200}) {
    std::vector<Pair> s = make(500, 3, k);
    std::reverse(s.begin(), s.end());
    check_stream("stream (descending index)", s, k);
  }
  if (g_failed) { std::fprintf(stderr, "knn_select_check: %d of %d cases FAILED\n", g_failed, g_cases); return 1; }
  std::printf("knn_select_check: %d cases ok\n", g_cases);
  return 0;
}
