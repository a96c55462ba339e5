// Selection rule of the k-NN search (csrc/knn.hip), as code that compiles for the device AND for the host: the kernels
// and tools/knn_select_check.cpp run the same lines.
//
// Total order of (score, bank index) pairs: higher score first, among equal scores the lower index first -- a STABLE
// descending sort of a query's score row (the rule vtx_cls_metrics documents for logits).  Indices are distinct, so the
// order is strict and the k first pairs are unique.
//
// A k-list is k pairs in that order.  Unused places hold the sentinel (-inf, KNN_NO_INDEX): every real pair -- bank
// indices stay below 2^31 - 1 -- comes before it, a NaN score is stored as -inf (knn_clean), so a list that has seen at
// least k pairs holds k real ones.
//
// Both updates are written per PLACE of the result, as pure functions of the old list(s): whoever owns place p (a lane of
// the wave that owns the row, a thread of the merge kernel, a loop iteration on the host) computes its new content from
// the unchanged input, and all places are written after all are computed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KNN_HD __host__ __device__ __forceinline__
#else
#define KNN_HD inline
#endif

#define KNN_NO_INDEX 0x7fffffff
#define KNN_MAX_K 256

KNN_HD float knn_neg_inf() { return -__builtin_huge_valf(); }

// a NaN score orders nowhere; it is kept as the lowest score so that the order stays total
KNN_HD float knn_clean(float s) { return s != s ? knn_neg_inf() : s; }

// pair a = (av, ai) comes before pair b = (bv, bi)
KNN_HD bool knn_before(float av, int32_t ai, float bv, int32_t bi) { return av > bv || (av == bv && ai < bi); }

// A candidate enters a full list exactly when it comes before the list's last pair.
KNN_HD bool knn_enters(float cv, int32_t ci, const float* val, const int32_t* idx, int k) {
  return knn_before(cv, ci, val[k - 1], idx[k - 1]);
}

// Place p of the list after candidate (cv, ci) has been inserted (the caller has checked knn_enters): the old pair while it
// comes before the candidate, the candidate at the first place whose old pair does not, the old left neighbour behind it.
KNN_HD void knn_insert_place(const float* val, const int32_t* idx, int p, float cv, int32_t ci, float* ov, int32_t* oi) {
  // (all four reads first and selects after: on the device they are in flight together and nothing branches)
  const int pl = p > 0 ? p - 1 : 0;
  const float v = val[p], lv = val[pl];
  const int32_t i = idx[p], li = idx[pl];
  const bool keep = knn_before(v, i, cv, ci);
  const bool here = p == 0 || knn_before(lv, li, cv, ci);
  *ov = keep ? v : (here ? cv : lv);
  *oi = keep ? i : (here ? ci : li);
}

// Number of pairs of the k-list (val, idx) that come before (cv, ci): binary search, the list is in order.
KNN_HD int knn_count_before(const float* val, const int32_t* idx, int k, float cv, int32_t ci) {
  int lo = 0, hi = k;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (knn_before(val[mid], idx[mid], cv, ci)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Merge of `nlist` k-lists (list s at val + s * k, idx + s * k) that hold disjoint index sets: the place of pair p of list s
// in the merged order = the pairs before it in its own list (p) plus those before it in every other list.  The pair belongs
// to the answer when that place is < k.  Sentinels of different lists tie with each other, but at least k real pairs
// come before each of them whenever the lists together have seen k pairs, so a sentinel's place is never < k.
KNN_HD int knn_merge_place(const float* val, const int32_t* idx, int nlist, int k, int s, int p) {
  const float cv = val[s * k + p];
  const int32_t ci = idx[s * k + p];
  int place = p;
  for (int t = 0; t < nlist; ++t)
    if (t != s) place += knn_count_before(val + t * k, idx + t * k, k, cv, ci);
  return place;
}

// ---- lists of the shards of a bank that is cut over ranks (vtx_knn_merge_lists)
// `nlist` RAGGED lists: list t holds lens[t] (0 .. k) real pairs in order at val + t * list_stride / idx + t * list_stride,
// and its indices are local to a shard whose row 0 is row bases[t] of the whole bank.  The order is the one above on
// (score, GLOBAL index = bases[t] + idx): higher score first, among equal scores the lower global index first.  Places at
// or beyond lens[t] are never read -- there are no sentinels to rely on, a list says how long it is.  Scores go through
// knn_clean as they are read (a NaN orders as -inf); the global index is formed in 64 bits, so that no input overflows it.

KNN_HD bool knn_before_global(float av, int64_t ag, float bv, int64_t bg) { return av > bv || (av == bv && ag < bg); }

// Number of the `len` pairs of an ordered list of shard `base` that come before (cv, cg): binary search, <= 9 steps.
KNN_HD int knn_count_before_global(const float* val, const int32_t* idx, int len, int32_t base, float cv, int64_t cg) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (knn_before_global(knn_clean(val[mid]), (int64_t)base + idx[mid], cv, cg)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Place of pair p (< lens[s]) of list s in the merged order: the pairs before it in its own list (p) plus those before
// it in every other list.  Shards hold disjoint global rows, so the order is strict and the places 0 .. sum(lens) - 1 are
// taken once each; the pair belongs to the answer when its place is < k.
KNN_HD int knn_merge_place_lists(const float* val, const int32_t* idx, const int32_t* lens, const int32_t* bases, int nlist,
                                 int64_t list_stride, int s, int p) {
  const float cv = knn_clean(val[s * list_stride + p]);
  const int64_t cg = (int64_t)bases[s] + idx[s * list_stride + p];
  int place = p;
  for (int t = 0; t < nlist; ++t)
    if (t != s) place += knn_count_before_global(val + t * list_stride, idx + t * list_stride, lens[t], bases[t], cv, cg);
  return place;
}
