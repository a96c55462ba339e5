// Label propagation for semi-supervised video object segmentation on frozen patch features (the DAVIS protocol of the
// DINO paper) on the device: a k-NN search restricted to a spatial neighbourhood that never writes an affinity matrix, the
// exp((score - best) / T) vote over soft labels, and the mask-overlap counts of the region similarity J.
//
//   labelprop_search_kernel  one 256-thread workgroup per (sequence, grid row y, strip of 16 consecutive queries x0 .. x0 + 15
//                       of that row).  All four waves hold the strip's MFMA A-operand fragments (registers while D allows it,
//                       otherwise re-read through L1 / L2) and each keeps its OWN k-list per query, in LDS (knn_select.h), the
//                       list's last pair -- the threshold -- in registers of the lanes that see the query's scores.  The
//                       tiles of the strip are the 16-key tiles [16 t, 16 t + 15] of the key rows y' in [y - radius,
//                       y + radius] (clipped to the grid) of every context slot that intersect [x0 - radius, x0 + 15 + radius]
//                       (clipped to the row), in the order (slot, key row, tile); wave v multiplies tiles v, v + 4, ...  No
//                       other tile is touched, so the work is proportional to the neighbourhood and no (n_ctx P) x P object
//                       exists anywhere.  Behind one barrier the four lists of a query, which hold disjoint keys, are merged
//                       by place (knn_merge_place).  (A 30 x 53 frame has 120 strips: four waves per strip rather than four
//                       strips per workgroup is what fills the chip at B = 1.)
//                       The key fragments are read STRAIGHT FROM GLOBAL MEMORY (L2): lane (key, group) loads its 16-byte
//                       pieces of key row (slot, y', 16 t + key), the fragments of tile t + 1 before the products of tile t.
//                       No key tile is staged in LDS and the one barrier is the one before the merge (DESIGN.md 7l says why).
//                       The chain is that of knn_search_kernel: v_mfma_f32_16x16x32_bf16 (bf16) or 8 x
//                       v_mfma_f32_16x16x4_f32 (fp32, exact) per 32 columns of D, chunks ascending, the same resident-chunk
//                       counts -- the score of a pair depends on its two rows only and is bit for bit what vtx_knn_topk
//                       returns for them.
//                       A score is masked BEFORE the threshold compare: the key column must exist (the tail of a ragged row),
//                       |x' - x| <= radius must hold for the score's own query, and the query must exist.  A masked score never
//                       enters a list.  A passing score is inserted by the whole wave through knn_insert_place.
//   labelprop_vote_kernel    one wave per query, lanes over the channels: w_i = expf((val_i - val_0) / T), the two sums in
//                       neighbour order in fp32, products and sums never contracted (the device of probe_sgd_kernel), one IEEE
//                       division.  An index outside [0, n_ctx P) -- the sentinel included -- is skipped, never dereferenced.
//   mask_overlap_kernel      one workgroup per (map, label): three integer counts, thread t over pixels t, t + 256, ..., then a
//                       fixed tree.  No atomics; the counts are written, not added to.
//
// Selection is "exactly k under a total order" (higher score first, among equal scores the lower index first).  The usual
// torch composition keeps EVERY key whose weight is >= the k-th largest, so it differs on exact ties at the k-th place, and
// only there.
//
// No floating-point atomics anywhere; plain vector stores only; the same inputs give the same bits.
#include "vtx_common.h"
#include "knn_select.h"

#include <math.h>

#define LP_MAX_CTX 16        // context slots of a call at most
#define LP_MAX_K 64
#define LP_MAX_D 1024
#define LP_MAX_C 1024        // channels of the soft labels at most
#define LP_MAX_LABELS 256    // labels vtx_mask_overlap counts at most

struct LpSlots { int32_t s[LP_MAX_CTX]; };             // by value: 64 B of kernel argument

// Keeps the compiler from moving one wave's LDS accesses across this point (csrc/knn.hip: knn_wave_sync).
__device__ __forceinline__ void lp_wave_sync() { asm volatile("" ::: "memory"); }

// value of lane b, b wave-uniform: v_readlane_b32
__device__ __forceinline__ float lp_lane_f(float v, int b) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), b));
}

// slots.s[c] through static indices: no scratch copy of the argument
__device__ __forceinline__ int lp_slot(const LpSlots& slots, int c) {
  int v = slots.s[0];
#pragma unroll
  for (int i = 1; i < LP_MAX_CTX; ++i) if (i == c) v = slots.s[i];
  return v;
}

// One candidate into the list (lv, li) of k <= 64 places, by the whole wave: lane p < k computes place p from the unchanged
// list, every lane also the last place, the query's new threshold (nt, ni); then all places are written.
__device__ __forceinline__ void lp_wave_insert(float* lv, int32_t* li, int k, float cv, int32_t ci, int lane, float& nt,
                                               int32_t& ni) {
  float nv;
  int32_t nx;
  knn_insert_place(lv, li, lane < k ? lane : k - 1, cv, ci, &nv, &nx);
  knn_insert_place(lv, li, k - 1, cv, ci, &nt, &ni);
  lp_wave_sync();
  if (lane < k) { lv[lane] = nv; li[lane] = nx; }
  lp_wave_sync();
}

// NCH > 0: the fragments of NCH 32-column chunks of D live in registers, the queries' for the whole kernel and the keys' one
// tile ahead (chunks past D are zero and add nothing); NCH == 0: any D, both are read where they are used (the parity path).
template <typename T, int NCH>
__global__ __launch_bounds__(256) void labelprop_search_kernel(const T* __restrict__ tar, const T* __restrict__ ctx,
                                                              float* __restrict__ out_val, int32_t* __restrict__ out_idx,
                                                              LpSlots slots, int n_ctx, int S, int h, int w, int D, int radius,
                                                              int k, int nstrips) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lp_smem[];
  float* lv = reinterpret_cast<float*>(lp_smem);                        // [16 queries][4 waves][k] list scores
  int32_t* li = reinterpret_cast<int32_t*>(lv + 64 * k);                // [16 queries][4 waves][k] list indices

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  const unsigned bid = blockIdx.x;
  const int strip = (int)(bid % (unsigned)nstrips);
  const unsigned rest = bid / (unsigned)nstrips;
  const int y = (int)(rest % (unsigned)h);
  const int64_t b = (int64_t)(rest / (unsigned)h);
  const int xw = strip * 16;                                            // first query column of the workgroup (< w)
  const int P = h * w;
  // list of query r of this wave: the four lists of a query lie side by side for the merge
  for (int e = lane; e < 16 * k; e += 64) {
    const int r = e / k, p = e - r * k;
    lv[(r * 4 + wave) * k + p] = knn_neg_inf();
    li[(r * 4 + wave) * k + p] = KNN_NO_INDEX;
  }
  lp_wave_sync();
  // thresholds of the queries whose scores this lane sees: query 4 g + r
  float tv[4];
  int32_t ti[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { tv[r] = knn_neg_inf(); ti[r] = KNN_NO_INDEX; }

  // query row of this lane's A fragments (queries past the row repeat its last token; their lists are never written out)
  const int xq = xw + col < w ? xw + col : w - 1;
  const T* qrow = tar + ((int64_t)b * P + (int64_t)y * w + xq) * D;
  constexpr int NR = NCH > 0 ? NCH : 1;
  Vec8<T> qf[NR];
  if constexpr (NCH > 0) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int kk = c * 32 + g * 8;
      qf[c] = load8_clamped<T>(qrow + (kk < D ? kk : 0), kk < D);
    }
  }

  const int y_lo = y - radius > 0 ? y - radius : 0, y_hi = y + radius < h - 1 ? y + radius : h - 1;
  const int x_lo = xw - radius > 0 ? xw - radius : 0, x_hi = xw + 15 + radius < w - 1 ? xw + 15 + radius : w - 1;
  const int t_lo = x_lo >> 4, t_hi = x_hi >> 4, ntx = t_hi - t_lo + 1;
  const int total = n_ctx * (y_hi - y_lo + 1) * ntx;                    // tiles of the workgroup, <= 16 * P
  const int nch = (D + 31) >> 5;

  // key row of this lane's B fragments in tile (c, yy, tx); a column past the row repeats its last token (masked below), a
  // tile behind the last one is the last one (loaded ahead, never multiplied)
  auto key_row = [&](int c, int yy, int tx) -> const T* {
    if (c >= n_ctx) { c = n_ctx - 1; yy = y_hi; tx = t_hi; }
    const int kx = tx * 16 + col < w ? tx * 16 + col : w - 1;
    return ctx + (((int64_t)b * S + lp_slot(slots, c)) * P + (int64_t)yy * w + kx) * D;
  };
  // the tiles in the order (slot, key row, key tile); wave v multiplies tiles v, v + 4, v + 8, ...
  int nc = 0, ny = y_lo, nt_ = t_lo;                                    // the wave's next tile
  auto advance = [&](int steps) {
    nt_ += steps;
    while (nt_ > t_hi) { nt_ -= ntx; if (++ny > y_hi) { ny = y_lo; ++nc; } }
  };
  advance(wave);
  Vec8<T> nf[NR];
  if constexpr (NCH > 0) {
    const T* kr = key_row(nc, ny, nt_);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int kk = c * 32 + g * 8;
      nf[c] = load8_clamped<T>(kr + (kk < D ? kk : 0), kk < D);
    }
  }

  for (int t = wave; t < total; t += 4) {
    const int c = nc, yy = ny, tx = nt_;
    advance(4);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (NCH > 0) {
      Vec8<T> bf[NCH];
#pragma unroll
      for (int cc = 0; cc < NCH; ++cc) bf[cc] = nf[cc];
      const T* kr = key_row(nc, ny, nt_);                               // the next tile's fragments: no branch around the loads
#pragma unroll
      for (int cc = 0; cc < NCH; ++cc) {
        const int kk = cc * 32 + g * 8;
        nf[cc] = load8_clamped<T>(kr + (kk < D ? kk : 0), kk < D);
      }
#pragma unroll
      for (int cc = 0; cc < NCH; ++cc) mma16(qf[cc], bf[cc], acc);
      acc_settle(acc);
    } else {
      const T* kr = key_row(c, yy, tx);
      for (int cc = 0; cc < nch; ++cc) {
        const int kk = cc * 32 + g * 8;
        const int ko = kk < D ? kk : 0;
        const Vec8<T> bf = load8_clamped<T>(kr + ko, kk < D);
        const Vec8<T> a = load8_clamped<T>(qrow + ko, kk < D);
        mma16(a, bf, acc);
        acc_settle(acc);                               // read in the block of the products (vtx_common.h)
      }
    }
    // ---- which scores are candidates and come before their query's last pair
    const int kx = tx * 16 + col;
    const int32_t cbase = c * P + yy * w + tx * 16;                     // index of the tile's key column 0
    const int32_t j = (int32_t)((uint32_t)cbase + (uint32_t)col);       // (a column past the row is masked; no signed wrap)
    unsigned pm = 0u;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc[r] = knn_clean(acc[r]);
      const int x = xw + 4 * g + r;
      const int dx = kx - x;
      if (kx < w && x < w && dx <= radius && -dx <= radius && knn_before(acc[r], j, tv[r], ti[r])) pm |= 1u << r;
    }
    if (__ballot(pm != 0u) != 0ull) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        unsigned long long mask = __ballot((pm >> r) & 1u);
        while (mask) {
          const int bl = __builtin_ctzll(mask);
          mask &= mask - 1;
          const float cv = lp_lane_f(acc[r], bl);
          const int32_t ci = cbase + (bl & 15);
          const float tvb = lp_lane_f(tv[r], bl);                       // the query's threshold now (an earlier pass of this
          const int32_t tib = __builtin_amdgcn_readlane(ti[r], bl);     // loop may have raised it)
          if (knn_before(cv, ci, tvb, tib)) {
            const int row = 4 * (bl >> 4) + r;
            float nt;
            int32_t ni;
            lp_wave_insert(lv + (row * 4 + wave) * k, li + (row * 4 + wave) * k, k, cv, ci, lane, nt, ni);
            if (g == (bl >> 4)) { tv[r] = nt; ti[r] = ni; }
          }
        }
      }
    }
  }

  // ---- the four lists of a query hold disjoint keys: every pair finds its place among all of them (knn_merge_place).
  // Fewer than k candidates: the sentinels of the four lists tie, land on the places behind the real pairs, and every such
  // place is written, with the same sentinel by whoever gets there.
  __syncthreads();
  for (int e = tid; e < 64 * k; e += 256) {
    const int r = e / (4 * k), rem = e - r * 4 * k;
    const int s = rem / k, p = rem - s * k;
    const int x = xw + r;
    if (x >= w) continue;
    const int place = knn_merge_place(lv + r * 4 * k, li + r * 4 * k, 4, k, s, p);
    if (place < k) {
      const int64_t base = ((int64_t)b * P + (int64_t)y * w + x) * k;
      out_val[base + place] = lv[e];
      out_idx[base + place] = li[e];
    }
  }
}

// ------------------------------------------------------------------------------------------------ vote
// A product as its own rounded value (csrc/probe.hip: probe_rounded): the backend does not fuse across the empty statement.
__device__ __forceinline__ float lp_rounded(float v) { asm volatile("" : "+v"(v)); return v; }

// Four queries per workgroup, one wave each; lane l forms channels l, l + 64, ...
__global__ __launch_bounds__(256) void labelprop_vote_kernel(const float* __restrict__ val, const int32_t* __restrict__ idx,
                                                            const float* __restrict__ seg, float* __restrict__ out,
                                                            LpSlots slots, int n_ctx, int S, int64_t BP, int P, int k, int C,
                                                            float T) {
#pragma clang fp contract(off)
  __shared__ float s_w[4][LP_MAX_K];
  __shared__ int64_t s_row[4][LP_MAX_K];               // row of seg (in rows of C floats) of neighbour i, -1: skipped
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t m = (int64_t)blockIdx.x * 4 + wave;
  const bool live = m < BP;
  if (live && lane < k) {
    const int64_t b = m / P;
    const float v0 = val[m * k];
    const float v = val[m * k + lane];
    const int32_t i = idx[m * k + lane];
    const bool ok = i >= 0 && (int64_t)i < (int64_t)n_ctx * P;
    const int c = ok ? i / P : 0;
    const int pp = ok ? i - c * P : 0;
    s_row[wave][lane] = ok ? ((int64_t)b * S + lp_slot(slots, c)) * P + pp : (int64_t)-1;
    const float d = v == v0 ? 0.f : v - v0;            // (equal scores, -inf included, weigh 1)
    s_w[wave][lane] = expf(d / T);
  }
  __syncthreads();
  if (!live) return;
  for (int c = lane; c < C; c += 64) {
    float num = 0.f, den = 0.f;
    for (int i = 0; i < k; ++i) {
      const int64_t row = s_row[wave][i];
      if (row < 0) continue;
      const float wi = s_w[wave][i];
      const float t = lp_rounded(wi * seg[row * C + c]);
      num = num + t;
      den = den + wi;
    }
    out[m * C + c] = den == 0.f ? 0.f : __fdiv_rn(num, den);
  }
}

// ------------------------------------------------------------------------------------------------ mask overlap
// blockIdx.x = map * C + label.  counts[map][label] = [#(pred == label & gt == label), #(pred == label), #(gt == label)].
__global__ __launch_bounds__(256) void mask_overlap_kernel(const int32_t* __restrict__ pred, const int32_t* __restrict__ gt,
                                                          int64_t* __restrict__ counts, int P, int C) {
  __shared__ int32_t red[3][256];
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.x / (unsigned)C;
  const int32_t c = (int32_t)(blockIdx.x % (unsigned)C);
  const int32_t* pr = pred + n * P;
  const int32_t* g = gt + n * P;
  int32_t both = 0, np = 0, ng = 0;                    // <= P < 2^31 each
  for (int i = tid; i < P; i += 256) {
    const bool a = pr[i] == c, bb = g[i] == c;
    both += (a && bb) ? 1 : 0;
    np += a ? 1 : 0;
    ng += bb ? 1 : 0;
  }
  red[0][tid] = both; red[1][tid] = np; red[2][tid] = ng;
  __syncthreads();
  for (int sft = 128; sft >= 1; sft >>= 1) {
    if (tid < sft) {
#pragma unroll
      for (int i = 0; i < 3; ++i) red[i][tid] += red[i][tid + sft];
    }
    __syncthreads();
  }
  if (tid < 3) counts[(int64_t)blockIdx.x * 3 + tid] = (int64_t)red[tid][0];
}

// ------------------------------------------------------------------------------------------------ host side
// The size rules the search and the vote share; fills `out` with the slots.
static int lp_ring_check(const int32_t* slots, int n_ctx, int S, int64_t B, int64_t P, LpSlots* out) {
  if (B < 1 || P < 1 || n_ctx < 1 || n_ctx > LP_MAX_CTX || S < 1) return VTX_ERR_SHAPE;
  for (int i = 0; i < LP_MAX_CTX; ++i) {
    out->s[i] = 0;
    if (i >= n_ctx) continue;
    if (slots[i] < 0 || slots[i] >= S) return VTX_ERR_SHAPE;
    out->s[i] = slots[i];
  }
  if (P >= (1ll << 31) || (int64_t)n_ctx * P >= (1ll << 31) - 1) return VTX_ERR_SHAPE;
  if (B >= (1ll << 31) || (int64_t)S * P >= (1ll << 31) || B * ((int64_t)S * P) >= (1ll << 31)) return VTX_ERR_SHAPE;
  return VTX_OK;
}

template <typename T, int NCH>
static void lp_launch(const void* tar, const void* ctx, float* val, int32_t* idx, const LpSlots& sl, int n_ctx, int S,
                      int64_t B, int h, int w, int D, int radius, int k, hipStream_t st) {
  const int nstrips = (w + 15) / 16;
  const unsigned grid = (unsigned)(B * h * nstrips);                     // <= B P < 2^31
  hipLaunchKernelGGL((labelprop_search_kernel<T, NCH>), dim3(grid), dim3(256), (size_t)64 * k * 8, st, (const T*)tar,
                     (const T*)ctx, val, idx, sl, n_ctx, S, h, w, D, radius, k, nstrips);
}

extern "C" {

/* include/vtx.h: vtx_labelprop_topk */
int vtx_labelprop_topk(const void* tar, const void* ctx, const int32_t* slots, int n_ctx, int S, float* val, int32_t* idx,
                       int64_t B, int h, int w, int D, int radius, int k, int dtype, void* stream) {
  if (!tar || !ctx || !slots || !val || !idx) return VTX_ERR_NULL;
  if (h < 1 || w < 1 || D < 1 || D > LP_MAX_D || k < 1 || k > LP_MAX_K || radius < 0) return VTX_ERR_SHAPE;
  LpSlots sl;
  const int rc = lp_ring_check(slots, n_ctx, S, B, (int64_t)h * w, &sl);
  if (rc != VTX_OK) return rc;
  if (dtype != VTX_BF16 && dtype != VTX_F32) return VTX_ERR_DTYPE;
  if (D % 8 != 0) return VTX_ERR_ALIGN;
  if (((uintptr_t)tar | (uintptr_t)ctx) & 15u) return VTX_ERR_ALIGN;
  if (((uintptr_t)val | (uintptr_t)idx) & 3u) return VTX_ERR_ALIGN;
  const int span = h > w ? h : w;
  const int rad = radius < span ? radius : span;       // restricts nothing from max(h, w) - 1 on; keeps y + radius in int
  hipStream_t st = (hipStream_t)stream;
  const int nch = (D + 31) / 32;
  // (the resident-chunk counts of vtx_knn_topk, so that a pair's chain is the same instruction sequence)
  if (dtype == VTX_BF16) {
    if (nch <= 4) lp_launch<bf16, 4>(tar, ctx, val, idx, sl, n_ctx, S, B, h, w, D, rad, k, st);
    else if (nch <= 12) lp_launch<bf16, 12>(tar, ctx, val, idx, sl, n_ctx, S, B, h, w, D, rad, k, st);
    else lp_launch<bf16, 0>(tar, ctx, val, idx, sl, n_ctx, S, B, h, w, D, rad, k, st);
  } else {
    if (nch <= 4) lp_launch<float, 4>(tar, ctx, val, idx, sl, n_ctx, S, B, h, w, D, rad, k, st);
    else lp_launch<float, 0>(tar, ctx, val, idx, sl, n_ctx, S, B, h, w, D, rad, k, st);
  }
  return vtx_check_launch();
}

/* include/vtx.h: vtx_labelprop_vote */
int vtx_labelprop_vote(const float* val, const int32_t* idx, const float* seg, const int32_t* slots, int n_ctx, int S,
                       float* out, int64_t B, int64_t P, int k, int C, float T, void* stream) {
  if (!val || !idx || !seg || !slots || !out) return VTX_ERR_NULL;
  if (C < 1 || C > LP_MAX_C || k < 1 || k > LP_MAX_K || !(T > 0.f) || !(T < INFINITY)) return VTX_ERR_SHAPE;
  LpSlots sl;
  const int rc = lp_ring_check(slots, n_ctx, S, B, P, &sl);
  if (rc != VTX_OK) return rc;
  if (((uintptr_t)val | (uintptr_t)idx | (uintptr_t)seg | (uintptr_t)out) & 3u) return VTX_ERR_ALIGN;
  const int64_t BP = B * P;                            // < 2^31
  hipLaunchKernelGGL(labelprop_vote_kernel, dim3((unsigned)((BP + 3) / 4)), dim3(256), 0, (hipStream_t)stream, val, idx, seg,
                     out, sl, n_ctx, S, BP, (int)P, k, C, T);
  return vtx_check_launch();
}

/* include/vtx.h: vtx_mask_overlap */
int vtx_mask_overlap(const int32_t* pred, const int32_t* gt, int64_t* counts, int64_t N, int64_t P, int C, void* stream) {
  if (!pred || !gt || !counts) return VTX_ERR_NULL;
  if (N < 1 || P < 1 || C < 1 || C > LP_MAX_LABELS || N >= (1ll << 31) || P >= (1ll << 31) || N * P >= (1ll << 31))
    return VTX_ERR_SHAPE;
  if (((uintptr_t)pred | (uintptr_t)gt) & 3u) return VTX_ERR_ALIGN;
  if ((uintptr_t)counts & 7u) return VTX_ERR_ALIGN;
  if (N * C >= (1ll << 31)) return VTX_ERR_SHAPE;      // (the grid; N P < 2^31 and C <= 256 leave this to tiny maps)
  hipLaunchKernelGGL(mask_overlap_kernel, dim3((unsigned)(N * C)), dim3(256), 0, (hipStream_t)stream, pred, gt, counts, (int)P,
                     C);
  return vtx_check_launch();
}

}  // extern "C"
