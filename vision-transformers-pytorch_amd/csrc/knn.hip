// Weighted k-nearest-neighbour evaluation of frozen features (the measure DINO runs are judged by) on the device:
// a fused search that never writes the (M, N) score matrix, and the exp(similarity / T) vote with its meter.
//
//   knn_search_kernel   one 256-thread workgroup per (bank split, tile of TM = 64 QB query rows; QB = 2 while k <= 64).
//                       Wave w owns query rows 16 QB w .. of the tile: their MFMA A-operand fragments stay resident
//                       (registers while D allows it, otherwise re-read through L1/L2) and so do their k-lists, in LDS
//                       (knn_select.h), with each list's last pair -- the row's threshold -- in registers of the lanes
//                       that see the row's scores.  The split's slab of the bank streams through ONE LDS tile of
//                       TN = 64 / 32 / 16 rows (the largest whose bytes fit 64 KiB): every thread loads its 16-byte
//                       pieces of tile t + 1 into registers before the products of tile t and stores them to LDS behind
//                       the barrier that ends those products.  Every wave multiplies its rows with the whole tile, 16
//                       bank rows at a time: v_mfma_f32_16x16x32_bf16 (bf16) or 8 x v_mfma_f32_16x16x4_f32 (fp32, exact)
//                       per 32 columns of D, the SAME chain for every pair -- the score of a pair depends on its two
//                       rows only, not on M, N, the tile or the split it falls in.
//                       A score is compared with its row's threshold in registers; one ballot per 16 x 16 QB scores
//                       says whether any passed.  A passing score is inserted by the whole wave, every lane computing
//                       the places it owns from the unchanged list (knn_insert_place) -- no other wave touches these
//                       rows, so nothing but the wave's own order is needed.  Past the first tiles a pass is rare
//                       (k / n of the scores at bank row n).
//   knn_merge_kernel    splits > 1: every split wrote its k-list to the workspace; one workgroup per query row places
//                       each of the splits * k pairs by counting the pairs before it (knn_merge_place).
//   knn_merge_lists_kernel   the bank is cut over ranks: every shard found a ragged list with shard-local indices; one
//                       workgroup per query row stages them in LDS and places each pair among all of them by global index
//                       (knn_merge_place_lists).  Serves the rank-major layout of a gather and the workspace layout.
//   knn_vote_kernel     one wave per query: w_i = expf(val_i / T), votes per class summed in neighbour order, the rank of
//                       the query's label and the winning class for up to 8 values of k.
//   knn_meter_kernel    one workgroup adds the batch to the fp64 meter in a fixed order (as cls_meter_accumulate_kernel).
//
// Grid order: blockIdx = split * query_tiles + query_tile, so the workgroups that run together read the same slab of the
// bank at about the same time: it comes from HBM once per XCD and from L2 / Infinity Cache for the other query tiles.
#include "vtx_common.h"
#include "knn_select.h"

#define KNN_TN_MAX 64        // bank rows of an LDS tile at most
#define KNN_STAGE 16         // 16-byte pieces of a bank tile a thread holds in flight (16 * 256 * 16 B = 64 KiB)
#define KNN_MAX_SPLITS 64
#define KNN_LDS_BYTES (160 * 1024)   // LDS of a CU: one workgroup may have all of it
#define KNN_MAX_D 1024

#define KNN_MAX_LISTS 64     // lists (shards) vtx_knn_merge_lists takes at most

struct KnnKs { int k[8]; };
struct KnnLists { int32_t len[KNN_MAX_LISTS]; int32_t base[KNN_MAX_LISTS]; };      // by value: 512 B of kernel argument

// Keeps the compiler from moving one wave's LDS accesses across this point.  Nothing is waited for: the lanes of a wave run
// in lockstep and LDS serves a wave's accesses in order.  (A fence would also wait for the bank tile's global loads that
// are in flight on purpose -- it cost the search most of its time.)
__device__ __forceinline__ void knn_wave_sync() { asm volatile("" ::: "memory"); }

// value of lane b, b wave-uniform: v_readlane_b32, no LDS round trip
__device__ __forceinline__ float knn_lane_f(float v, int b) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), b));
}

// One candidate into row list (lv, li), by the whole wave: each lane computes the places p = lane, lane + 64, .. it owns
// from the unchanged list -- every lane also the last place, the row's new threshold (nt, ni) -- then all places are
// written.  LDS serves one wave's accesses in order, so the next insert of this wave reads the new list.
__device__ __forceinline__ void knn_wave_insert(float* lv, int32_t* li, int k, float cv, int32_t ci, int lane, float& nt,
                                                int32_t& ni) {
  float nv[KNN_MAX_K / 64];
  int32_t nx[KNN_MAX_K / 64];
#pragma unroll
  for (int i = 0; i < KNN_MAX_K / 64; ++i) {
    const int p = lane + 64 * i;
    nv[i] = 0.f; nx[i] = 0;
    if (64 * i < k) knn_insert_place(lv, li, p < k ? p : k - 1, cv, ci, &nv[i], &nx[i]);      // (wave-uniform skip)
  }
  knn_insert_place(lv, li, k - 1, cv, ci, &nt, &ni);
  knn_wave_sync();
#pragma unroll
  for (int i = 0; i < KNN_MAX_K / 64; ++i) {
    const int p = lane + 64 * i;
    if (p < k) { lv[p] = nv[i]; li[p] = nx[i]; }
  }
  knn_wave_sync();
}

// NCH > 0: the query fragments of NCH 32-column chunks of D live in registers (chunks past D are zero and add nothing);
// NCH == 0: any D, the fragments are re-read from global memory for every bank tile (the parity path).
template <typename T, int NCH, int QB>
__global__ __launch_bounds__(256) void knn_search_kernel(const T* __restrict__ q, const T* __restrict__ f,
                                                        float* __restrict__ out_val, int32_t* __restrict__ out_idx, int M,
                                                        int N, int D, int k, int nqt, int splits, int per, int TN, int nwq) {
  extern __shared__ __attribute__((aligned(16))) unsigned char knn_smem[];
  constexpr int ES = (int)sizeof(T);
  const int TM = 16 * QB * nwq;                                         // query rows of the workgroup: nwq = 4 (or 2) waves own rows
  constexpr int WR = 16 * QB;                                           // query rows of a wave
  float* lv = reinterpret_cast<float*>(knn_smem);                       // [TM][k] list scores
  int32_t* li = reinterpret_cast<int32_t*>(lv + TM * k);                // [TM][k] list bank indices
  unsigned char* bt = reinterpret_cast<unsigned char*>(li + TM * k);    // [TN][pitch] the bank tile (TM k 8 is a multiple of 16)
  const int pitch = D * ES + 16;                                        // +16 B: rows 16 B apart in the 256-B bank row

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int qt = (int)(blockIdx.x % (unsigned)nqt), sp = (int)(blockIdx.x / (unsigned)nqt);
  const int m0 = qt * TM + wave * WR;                                   // first query row of this wave
  const int64_t nb64 = (int64_t)sp * per;
  const int n_beg = nb64 < (int64_t)N ? (int)nb64 : N;
  const int n_end = nb64 + per < (int64_t)N ? (int)(nb64 + per) : N;
  const int ntiles = (n_end - n_beg + TN - 1) / TN;
  const int nch = (D + 31) >> 5;
  const int nblk = TN >> 4;
  const bool qwave = wave < nwq;                                        // (the other waves only help to move the bank tile)
  float* wlv = lv + wave * WR * k;                                      // this wave's lists
  int32_t* wli = li + wave * WR * k;

  if (qwave)
    for (int e = lane; e < WR * k; e += 64) { wlv[e] = knn_neg_inf(); wli[e] = KNN_NO_INDEX; }
  // thresholds of the rows whose scores this lane sees: row qb * 16 + 4 g + r of the wave
  float tv[QB][4];
  int32_t ti[QB][4];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb)
#pragma unroll
    for (int r = 0; r < 4; ++r) { tv[qb][r] = knn_neg_inf(); ti[qb][r] = KNN_NO_INDEX; }

  // query rows of this lane's A fragments (rows past M repeat row M - 1; their lists are never written out)
  const T* qrow[QB];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    int r = m0 + qb * 16 + col;
    if (r > M - 1) r = M - 1;
    qrow[qb] = q + (int64_t)r * D;
  }
  Vec8<T> qf[QB][NCH > 0 ? NCH : 1];
  if constexpr (NCH > 0) {
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int kk = c * 32 + g * 8;
        qf[qb][c] = load8_clamped<T>(qrow[qb] + (kk < D ? kk : 0), kk < D);
      }
  }

  // this thread's 16-byte pieces of a bank tile: piece v = tid + 256 i is bytes [16 pc, 16 pc + 16) of tile row pr
  const int vpr = (D * ES) >> 4;
  const int nvec = TN * vpr;
  const int pr0 = tid / vpr, pc0 = tid - pr0 * vpr, dpr = 256 / vpr, dpc = 256 - dpr * vpr;
  uint4 st[KNN_STAGE];

  // tt = -1 only brings tile 0 in
  for (int tt = -1; tt < ntiles; ++tt) {
    const int row0 = n_beg + tt * TN;
    const bool more = tt + 1 < ntiles;
    if (more) {
      int pr = pr0, pc = pc0;
#pragma unroll
      for (int i = 0; i < KNN_STAGE; ++i) {
        int gr = row0 + TN + pr;
        if (gr > N - 1) gr = N - 1;                    // rows past the bank repeat its last row; their scores are masked
        const uint4* src = reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(f) + (int64_t)gr * (D * ES) + pc * 16);
        st[i] = tid + 256 * i < nvec ? *src : uint4{0u, 0u, 0u, 0u};
        pr += dpr; pc += dpc;
        if (pc >= vpr) { pc -= vpr; pr += 1; }
      }
    }

    if (tt >= 0 && qwave) {
      for (int blk = 0; blk < nblk; ++blk) {
        // ---- this wave's query rows x bank rows row0 + 16 blk .. + 15
        f32x4 acc[QB];
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) acc[qb] = f32x4{0.f, 0.f, 0.f, 0.f};
        const unsigned char* brow = bt + (blk * 16 + col) * pitch;
        if constexpr (NCH > 0) {
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            const int kk = c * 32 + g * 8;
            const Vec8<T> bf = load8_clamped<T>(reinterpret_cast<const T*>(brow) + (kk < D ? kk : 0), kk < D);
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) mma16(qf[qb][c], bf, acc[qb]);
          }
#pragma unroll
          for (int qb = 0; qb < QB; ++qb) acc_settle(acc[qb]);
        } else {
          for (int c = 0; c < nch; ++c) {
            const int kk = c * 32 + g * 8;
            const int ko = kk < D ? kk : 0;
            const Vec8<T> bf = load8_clamped<T>(reinterpret_cast<const T*>(brow) + ko, kk < D);
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
              const Vec8<T> a = load8_clamped<T>(qrow[qb] + ko, kk < D);
              mma16(a, bf, acc[qb]);
              acc_settle(acc[qb]);                     // read in the block of the products (vtx_common.h)
            }
          }
        }
        // ---- which scores come before their row's last pair
        const int j = row0 + blk * 16 + col;
        unsigned pm = 0u;
#pragma unroll
        for (int qb = 0; qb < QB; ++qb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            acc[qb][r] = knn_clean(acc[qb][r]);
            if (j < n_end && knn_before(acc[qb][r], j, tv[qb][r], ti[qb][r])) pm |= 1u << (qb * 4 + r);
          }
        if (__ballot(pm != 0u) != 0ull) {
#pragma unroll
          for (int qb = 0; qb < QB; ++qb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              unsigned long long mask = __ballot((pm >> (qb * 4 + r)) & 1u);
              while (mask) {
                const int b = __builtin_ctzll(mask);
                mask &= mask - 1;
                const float cv = knn_lane_f(acc[qb][r], b);
                const int32_t ci = row0 + blk * 16 + (b & 15);
                const float tvb = knn_lane_f(tv[qb][r], b);             // the row's threshold now (an earlier pass of this
                const int32_t tib = __builtin_amdgcn_readlane(ti[qb][r], b);      // loop may have raised it)
                if (knn_before(cv, ci, tvb, tib)) {
                  const int row = qb * 16 + 4 * (b >> 4) + r;
                  float nt;
                  int32_t ni;
                  knn_wave_insert(wlv + row * k, wli + row * k, k, cv, ci, lane, nt, ni);
                  if (g == (b >> 4)) { tv[qb][r] = nt; ti[qb][r] = ni; }
                }
              }
            }
        }
      }
    }
    __syncthreads();                                   // every wave is done with the tile
    if (more) {
      int pr = pr0, pc = pc0;
#pragma unroll
      for (int i = 0; i < KNN_STAGE; ++i) {
        if (tid + 256 * i < nvec) *reinterpret_cast<uint4*>(bt + pr * pitch + pc * 16) = st[i];
        pr += dpr; pc += dpc;
        if (pc >= vpr) { pc -= vpr; pr += 1; }
      }
    }
    __syncthreads();                                   // the next tile is in place
  }

  // ---- the lists of this split: every wave writes its rows
  for (int r = 0; r < WR; ++r) {
    const int m = m0 + r;
    if (m >= M || !qwave) break;
    const int64_t base = ((int64_t)m * splits + sp) * k;
    for (int p = lane; p < k; p += 64) {
      out_val[base + p] = wlv[r * k + p];
      out_idx[base + p] = wli[r * k + p];
    }
  }
}

// splits k-lists of query row m (workspace) -> its k-list
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ wv, const int32_t* __restrict__ wi,
                                                       float* __restrict__ val, int32_t* __restrict__ idx, int splits,
                                                       int k, int N) {
  const int64_t m = blockIdx.x;
  const float* v = wv + m * splits * k;
  const int32_t* ix = wi + m * splits * k;
  for (int e = threadIdx.x; e < splits * k; e += 256) {
    const int s = e / k, p = e - s * k;
    const int place = knn_merge_place(v, ix, splits, k, s, p);
    if (place < k) {
      int32_t i = ix[e];
      if (i > N - 1) i = N - 1;                        // (never taken while the order is total: the range promise)
      val[m * k + place] = v[e];
      idx[m * k + place] = i;
    }
  }
}

// The ragged lists of query row m that the shards of a bank cut over ranks found (list s: len[s] ordered pairs with indices
// local to a shard that starts at global row base[s]) -> the row's k-list with global indices.  One workgroup per query.
// The lists are staged in LDS as [nlist][k] (scores cleaned on the way in, places past len[s] left unwritten and never
// read) together with len and base: every pair is then read about nlist * log2(k) times by the binary searches of
// knn_merge_place_lists, and the kernel argument is indexed by the thread id once, in the staging loop.
__global__ __launch_bounds__(256) void knn_merge_lists_kernel(const float* __restrict__ lval, const int32_t* __restrict__ lidx,
                                                             float* __restrict__ val, int32_t* __restrict__ idx,
                                                             KnnLists lists, int nlist, int k, int64_t row_stride,
                                                             int64_t list_stride, int N) {
  extern __shared__ __attribute__((aligned(16))) unsigned char knn_smem[];
  __shared__ int32_t s_len[KNN_MAX_LISTS], s_base[KNN_MAX_LISTS];
  float* sv = reinterpret_cast<float*>(knn_smem);                       // [nlist][k]
  int32_t* si = reinterpret_cast<int32_t*>(sv + nlist * k);             // [nlist][k]
  const int64_t m = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid < KNN_MAX_LISTS) {
    s_len[tid] = tid < nlist ? lists.len[tid] : 0;
    s_base[tid] = tid < nlist ? lists.base[tid] : 0;
  }
  __syncthreads();
  const int total = nlist * k;
  for (int e = tid; e < total; e += 256) {
    const int s = e / k, p = e - s * k;
    if (p < s_len[s]) {
      const int64_t src = m * row_stride + s * list_stride + p;
      sv[e] = knn_clean(lval[src]);
      si[e] = lidx[src];
    }
  }
  __syncthreads();
  for (int e = tid; e < total; e += 256) {
    const int s = e / k, p = e - s * k;
    if (p >= s_len[s]) continue;
    const int place = knn_merge_place_lists(sv, si, s_len, s_base, nlist, k, s, p);
    if (place < k) {
      int64_t g = (int64_t)s_base[s] + si[e];
      g = g < 0 ? 0 : (g > N - 1 ? N - 1 : g);         // (never taken on the lists of a search: the range promise)
      val[m * k + place] = sv[e];
      idx[m * k + place] = (int32_t)g;
    }
  }
}

// ------------------------------------------------------------------------------------------------ vote
__device__ __forceinline__ int knn_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int knn_wave_min(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const int u = __shfl_xor(v, o, 64); v = u < v ? u : v; }
  return v;
}

// One wave per query.  w[i] = expf(val[i] / T); the vote of class c at k is the sum of w[i], i < k, lab[i] == c, taken in
// ascending i.  Only classes that own a neighbour have a sum to form; the others have vote 0 and enter the rank and the
// winner by count (rank) or as the lowest class without a neighbour (winner).  The lane that owns neighbour p forms the
// vote of lab[p] when p is the first neighbour of that class.
__global__ __launch_bounds__(64) void knn_vote_kernel(const float* __restrict__ val, const int32_t* __restrict__ idx,
                                                     const int64_t* __restrict__ bank_labels,
                                                     const int64_t* __restrict__ qlabels, int32_t* __restrict__ rank,
                                                     int32_t* __restrict__ pred, KnnKs ks, int nk, int L, int N, int C,
                                                     float T) {
  __shared__ float w[KNN_MAX_K];
  __shared__ int32_t lab[KNN_MAX_K];                   // class in [0, C), or -1: a label that is no class
  const int64_t m = blockIdx.x;
  const int lane = threadIdx.x;
  for (int p = lane; p < L; p += 64) {
    const int32_t i = idx[m * L + p];
    int64_t lb = (i >= 0 && i < N) ? bank_labels[i] : -1;
    lab[p] = (lb >= 0 && lb < (int64_t)C) ? (int32_t)lb : -1;
    w[p] = expf(val[m * L + p] / T);
  }
  __syncthreads();
  bool first[KNN_MAX_K / 64];
#pragma unroll
  for (int i = 0; i < KNN_MAX_K / 64; ++i) {
    const int p = lane + 64 * i;
    bool fo = p < L && lab[p] >= 0;
    if (fo) {
      const int32_t c = lab[p];
      for (int jn = 0; jn < p; ++jn) if (lab[jn] == c) { fo = false; break; }
    }
    first[i] = fo;
  }
  const int64_t ql = qlabels[m];
  const bool lvalid = ql >= 0 && ql < (int64_t)C;
  const int32_t l = lvalid ? (int32_t)ql : -1;

#pragma unroll 1
  for (int ki = 0; ki < nk; ++ki) {
    int k = ks.k[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) if (i == ki) k = ks.k[i];      // (static indices: no scratch copy of the argument)
    float vl = 0.f;                                    // the label's vote (0 without a neighbour)
    for (int jn = 0; jn < k; ++jn) if (lab[jn] == l && lvalid) vl += w[jn];
    int above = 0, present = 0, present_below = 0;
    float bv = -1.f;                                   // best class among this lane's: votes are >= 0
    int32_t bc = KNN_NO_INDEX;
#pragma unroll
    for (int i = 0; i < KNN_MAX_K / 64; ++i) {
      const int p = lane + 64 * i;
      if (first[i] && p < k) {
        const int32_t c = lab[p];
        float vc = 0.f;
        for (int jn = p; jn < k; ++jn) if (lab[jn] == c) vc += w[jn];
        present += 1;
        if (lvalid) {
          above += knn_before(vc, c, vl, l) ? 1 : 0;
          present_below += c < l ? 1 : 0;
        }
        if (bc == KNN_NO_INDEX || knn_before(vc, c, bv, bc)) { bv = vc; bc = c; }
      }
    }
    above = knn_wave_sum(above);
    present = knn_wave_sum(present);
    present_below = knn_wave_sum(present_below);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ov = shfl_xor_f(bv, o);
      const int32_t oc = __shfl_xor(bc, o, 64);
      if (oc != KNN_NO_INDEX && (bc == KNN_NO_INDEX || knn_before(ov, oc, bv, bc))) { bv = ov; bc = oc; }
    }
    // classes without a neighbour: vote 0
    int rk = C;                                        // a label that is no class: counted, never a hit
    if (lvalid) rk = above + (vl == 0.f ? l - present_below : 0);
    int32_t win = bc;
    if (present < C && (bc == KNN_NO_INDEX || !(bv > 0.f))) {
      // the lowest class without a neighbour is among the first present + 1 classes
      const int lim = present + 1 < C ? present + 1 : C;
      int amin = KNN_NO_INDEX;
      for (int c = lane; c < lim; c += 64) {
        bool has = false;
        for (int jn = 0; jn < k; ++jn) if (lab[jn] == c) { has = true; break; }
        if (!has && c < amin) amin = c;
      }
      amin = knn_wave_min(amin);
      if (amin != KNN_NO_INDEX && (bc == KNN_NO_INDEX || knn_before(0.f, amin, bv, bc))) win = amin;
    }
    if (lane == 0) { rank[m * nk + ki] = rk; pred[m * nk + ki] = win; }
  }
}

// meter[0] += M, meter[1 + 2 i] += rows with rank < 1, meter[2 + 2 i] += rows with rank < min(5, ks[i]).  Thread t sums
// rows t, t + 256, ... in fp64, then a fixed tree over the 256 partials.
__global__ __launch_bounds__(256) void knn_meter_kernel(const int32_t* __restrict__ rank, double* __restrict__ meter,
                                                       KnnKs ks, int nk, int M) {
  __shared__ double red[16][256];
  const int tid = threadIdx.x;
  double hits[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) hits[i] = 0.0;
  for (int m = tid; m < M; m += 256) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i < nk) {
        const int r = rank[(int64_t)m * nk + i];
        const int k5 = ks.k[i] < 5 ? ks.k[i] : 5;
        if (r < 1) hits[2 * i] += 1.0;
        if (r < k5) hits[2 * i + 1] += 1.0;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) red[i][tid] = hits[i];
  __syncthreads();
  for (int sft = 128; sft >= 1; sft >>= 1) {
    if (tid < sft) {
#pragma unroll
      for (int i = 0; i < 16; ++i) red[i][tid] += red[i][tid + sft];
    }
    __syncthreads();
  }
  if (tid == 0) meter[0] += (double)M;
  if (tid < 2 * nk) meter[1 + tid] += red[tid][0];
}

// ------------------------------------------------------------------------------------------------ host side
// Query rows of a workgroup: 128 (two 16-row blocks per wave) while the lists are short enough to leave the bank tile its
// LDS at any D, 64 otherwise.  A function of M and k alone, so that the workspace can be sized without D.
static int knn_tile_rows(int64_t M, int k) { return (k <= 64 && M > 64) ? 128 : 64; }

static int knn_resolve_splits(int64_t M, int64_t N, int k, int splits) {
  if (splits > 0) return splits;
  // as many workgroups as fit the 256 CUs in ONE round (one workgroup holds a CU's LDS; a second, part-filled round would
  // double the time), no split below 4096 bank rows
  const int TM = knn_tile_rows(M, k);
  const int64_t nqt = (M + TM - 1) / TM;
  int64_t s = 256 / nqt;
  const int64_t cap = N / 4096;
  if (s > cap) s = cap;
  if (s > KNN_MAX_SPLITS) s = KNN_MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}

static int knn_shape_check(int64_t M, int64_t N, int D, int k, int splits) {
  if (M < 1 || N < 1 || M >= (1ll << 31) || N >= (1ll << 31) || D < 1 || D > KNN_MAX_D || k < 1 || k > KNN_MAX_K ||
      (int64_t)k > N || splits < 0 || splits > KNN_MAX_SPLITS)
    return VTX_ERR_SHAPE;
  if (D % 8 != 0) return VTX_ERR_ALIGN;
  return VTX_OK;
}

template <typename T, int NCH, int QB>
static int knn_launch(const void* q, const void* f, float* ov, int32_t* oi, int M, int N, int D, int k, int nqt, int splits,
                      int per, int TN, int nwq, size_t smem, hipStream_t st) {
  auto kern = knn_search_kernel<T, NCH, QB>;
  if (smem > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
    return VTX_ERR_LAUNCH;
  hipLaunchKernelGGL(kern, dim3((unsigned)(nqt * splits)), dim3(256), smem, st, (const T*)q, (const T*)f, ov, oi, M, N, D, k,
                     nqt, splits, per, TN, nwq);
  return VTX_OK;
}

extern "C" {

/* include/vtx.h: vtx_knn_workspace_bytes */
size_t vtx_knn_workspace_bytes(int64_t M, int64_t N, int k, int splits) {
  if (knn_shape_check(M, N, 8, k, splits) != VTX_OK) return 0;
  const int s = knn_resolve_splits(M, N, k, splits);
  return s > 1 ? (size_t)M * (size_t)s * (size_t)k * 8u : 0;
}

/* include/vtx.h: vtx_knn_topk */
int vtx_knn_topk(const void* q, const void* f, float* val, int32_t* idx, int64_t M, int64_t N, int D, int k, int splits,
                 void* ws, size_t ws_bytes, int dtype, void* stream) {
  if (!q || !f || !val || !idx) return VTX_ERR_NULL;
  const int rc = knn_shape_check(M, N, D, k, splits);
  if (rc != VTX_OK) return rc;
  if (dtype != VTX_BF16 && dtype != VTX_F32) return VTX_ERR_DTYPE;
  if (((uintptr_t)q | (uintptr_t)f) & 15u) return VTX_ERR_ALIGN;
  const int s = knn_resolve_splits(M, N, k, splits);
  const size_t need = s > 1 ? (size_t)M * (size_t)s * (size_t)k * 8u : 0;
  if (need > 0) {
    if (ws_bytes < need) return VTX_ERR_WORKSPACE;
    if (!ws) return VTX_ERR_NULL;
    if ((uintptr_t)ws & 3u) return VTX_ERR_ALIGN;
  }

  const int es = dtype == VTX_BF16 ? 2 : 4;
  // tile shape: the nominal query tile with the largest bank tile of at most 64 KiB that leaves the lists their LDS; where
  // not even 16 bank rows fit beside 64 lists (k and D both near their limits), two waves own 16 rows each
  const int QB = knn_tile_rows(M, k) / 64;
  int nwq = 0, TN = 0;
  size_t smem = 0;
  for (int w = 4; w >= 2 && TN == 0; w -= 2)
    for (int tn = KNN_TN_MAX; tn >= 16 && TN == 0; tn >>= 1) {
      const size_t need_lds = (size_t)16 * QB * w * k * 8 + (size_t)tn * (D * es + 16);
      if (tn * D * es <= 65536 && need_lds <= KNN_LDS_BYTES) { TN = tn; nwq = w; smem = need_lds; }
    }
  if (TN == 0) return VTX_ERR_SHAPE;                   // (not reached within the limits above: 64 KiB + 64.25 KiB fit)
  const int TM = 16 * QB * nwq;
  const int nqt = (int)((M + TM - 1) / TM);
  if ((int64_t)nqt * s >= (1ll << 31)) return VTX_ERR_SHAPE;
  const int per = (int)((N + s - 1) / s);
  float* ov = s > 1 ? (float*)ws : val;
  int32_t* oi = s > 1 ? (int32_t*)((float*)ws + (size_t)M * s * k) : idx;
  hipStream_t st = (hipStream_t)stream;
  const int nch = (D + 31) / 32;
  int lr;
#define KNN_GO(T, NCH, QB) lr = knn_launch<T, NCH, QB>(q, f, ov, oi, (int)M, (int)N, D, k, nqt, s, per, TN, nwq, smem, st)
  if (dtype == VTX_BF16) {
    if (QB == 2) { if (nch <= 4) KNN_GO(bf16, 4, 2); else if (nch <= 12) KNN_GO(bf16, 12, 2); else KNN_GO(bf16, 0, 2); }
    else { if (nch <= 4) KNN_GO(bf16, 4, 1); else if (nch <= 12) KNN_GO(bf16, 12, 1); else KNN_GO(bf16, 0, 1); }
  } else {
    if (QB == 2) { if (nch <= 4) KNN_GO(float, 4, 2); else KNN_GO(float, 0, 2); }
    else { if (nch <= 4) KNN_GO(float, 4, 1); else KNN_GO(float, 0, 1); }
  }
#undef KNN_GO
  if (lr != VTX_OK) return lr;
  if (s > 1)
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)M), dim3(256), 0, st, (const float*)ov, (const int32_t*)oi, val, idx,
                       s, k, (int)N);
  return vtx_check_launch();
}

/* include/vtx.h: vtx_knn_merge_lists */
int vtx_knn_merge_lists(const float* lval, const int32_t* lidx, float* val, int32_t* idx, const int32_t* lens,
                        const int32_t* bases, int nlist, int64_t M, int k, int64_t row_stride, int64_t list_stride, int64_t N,
                        void* stream) {
  if (!lval || !lidx || !val || !idx || !lens || !bases) return VTX_ERR_NULL;
  if (M < 1 || M >= (1ll << 31) || N < 1 || N >= (1ll << 31) - 1 || nlist < 1 || nlist > KNN_MAX_LISTS || k < 1 ||
      k > KNN_MAX_K)
    return VTX_ERR_SHAPE;
  KnnLists L;
  int64_t sum = 0;
  for (int s = 0; s < KNN_MAX_LISTS; ++s) {
    L.len[s] = 0; L.base[s] = 0;
    if (s >= nlist) continue;
    const int64_t lo = bases[s], hi = s + 1 < nlist ? (int64_t)bases[s + 1] : N;      // shard s holds global rows [lo, hi)
    if (lo < 0 || hi < lo || lens[s] < 0 || lens[s] > k || (int64_t)lens[s] > hi - lo) return VTX_ERR_SHAPE;
    L.len[s] = lens[s]; L.base[s] = bases[s];
    sum += lens[s];
  }
  if (sum < k) return VTX_ERR_SHAPE;
  if ((nlist > 1 && list_stride < k) || (M > 1 && row_stride < k)) return VTX_ERR_SHAPE;
  const size_t smem = (size_t)nlist * k * 8;           // <= 128 KiB
  if (smem + 512 > 64 * 1024 && hipFuncSetAttribute((const void*)knn_merge_lists_kernel,      // (+ the 512 B of len / base)
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
    return VTX_ERR_LAUNCH;
  hipLaunchKernelGGL(knn_merge_lists_kernel, dim3((unsigned)M), dim3(256), smem, (hipStream_t)stream, lval, lidx, val, idx, L,
                     nlist, k, row_stride, list_stride, (int)N);
  return vtx_check_launch();
}

/* include/vtx.h: vtx_knn_vote */
int vtx_knn_vote(const float* val, const int32_t* idx, const int64_t* bank_labels, const int64_t* query_labels,
                 int32_t* rank, int32_t* pred, double* meter, const int32_t* ks, int nk, int64_t M, int L, int64_t N, int C,
                 float T, void* stream) {
  if (!val || !idx || !bank_labels || !query_labels || !rank || !pred || !ks) return VTX_ERR_NULL;
  if (M < 1 || M >= (1ll << 31) || N < 1 || N >= (1ll << 31) || L < 1 || L > KNN_MAX_K || C < 1 || nk < 1 || nk > 8 ||
      !(T > 0.f))
    return VTX_ERR_SHAPE;
  KnnKs kk;
  for (int i = 0; i < 8; ++i) {
    kk.k[i] = i < nk ? ks[i] : 1;
    if (i < nk && (ks[i] < 1 || ks[i] > L)) return VTX_ERR_SHAPE;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)M), dim3(64), 0, st, val, idx, bank_labels, query_labels, rank, pred, kk,
                     nk, L, (int)N, C, T);
  if (meter)
    hipLaunchKernelGGL(knn_meter_kernel, dim3(1), dim3(256), 0, st, (const int32_t*)rank, meter, kk, nk, (int)M);
  return vtx_check_launch();
}

}  // extern "C"
