// Read-only inspection of global attention: rows of P = softmax(q k^T / sqrt(D)), per-query attention statistics without writing P, a
// per-(layer, head) fp64 meter over them, and the mass threshold of DINO's attention visualisation.  In the reference the attention
// probabilities are an ordinary tensor (models/vit.py:36-39) that a hook can read; here no kernel stores them, so these entries
// recompute them from the operands the attention kernels take.
//
// Operands as vtx_attn_hd_fwd (csrc/attention_hd.hip): q [B * Lq, nH * D] with row stride ldq, k [B * Lk, nH * D] with row stride
// ldkv -- the packed QKV projection (ldq = ldkv = 3 nH D) or the q | kv pair of PVT / Twins -- bf16 or fp32, D any multiple of 8 in
// 8..128 (templated on the padded width DP in {32, 64, 96, 128}; the PADDING RULE of attention_hd.hip holds: a vector at d0 >= D is a
// zero operand whose memory is never touched).  No bias, no mask, no windows in vtx_attn_map_*; window and halo attention (Swin, the
// Twins locally-grouped half, Halo) take the same kernels through vtx_attn_mapw_* (WINDOW AND HALO ATTENTION, below).
//
// SCORES.  s(q, key) = acc * scale with acc the MFMA chain of hdattn_fwd_kernel -- one v_mfma_f32_16x16x32_bf16 per 32 columns in
// bf16, eight v_mfma_f32_16x16x4_f32 per 32 columns (the exact fmaf chain) in fp32, fp32 accumulation -- and scale the fp32
// 1.0f / sqrtf((float)D): ONE fp32 multiply.  A wave owns 16 queries; a product gives S^T[key][query]: lane (c = lane & 15,
// g = lane >> 4) holds, for query c of the wave, the keys k0 + 16 kt + 4 g + r (kt, r in 0..3) of the key block k0 .. k0 + 63.  The
// K fragments come from global memory (L2) as in hdattn_fwd_kernel; nothing is staged in LDS and the kernels have no barrier.  An
// output element depends on its own query row and key rows alone, so a row's outputs are the same bits wherever the row lands in a
// tile: however the rows are cut into calls (row0 / nrows), however the batch is cut, packed or split operands.
//
// BOTH score kernels make passes over the key blocks, K re-read from L2, instead of rescaling running sums (the issue's other
// choice): the row maximum is then exact and the sums are taken against the final maximum only.
//   pass 1   m = max_j s_j.  Per lane over its keys (padded keys count as -inf), then fmaxf with lane ^ 16 and lane ^ 32.  A maximum
//            does not depend on the order: smax = m is the largest scaled logit bit for bit.
//   pass 2   e_j = __expf(s_j - m) for the lane's keys j < Lk, in the order key block, kt, r; per lane, each starting from 0.f:
//              l  += e_j                 es += e_j * s_j
//              ep += e_j  if j < n_prefix              ed += e_j * dist(i, j)  if j >= n_prefix and i >= n_prefix
//            (hipcc may contract each product and sum into one fma: the envelope charges the sum, which covers both).  Then the four
//            lanes of a query meet once, in a fixed butterfly:  x += x(lane ^ 16);  x += x(lane ^ 32)  for l, es, ep, ed.
//   dist(i, j) = v_sqrt_f32((float)(dy * dy + dx * dx)) with dy, dx the integer row / column differences of the grid positions
//            ((t - n_prefix) / gw, (t - n_prefix) % gw); the argument is an exact integer below 2^24, the instruction is within 1 ulp.
//   vtx_attn_map_stats stores, per query row i (fp32 [B, nH, Lq, 5]):
//              lse = m + __logf(l)       entropy = lse - es / l       smax = m       prefix = ep / l       dist = ed / l
//            (IEEE divisions).  dist is 0.f for a prefix query row and with gh = gw = 0.
//   vtx_attn_map_rows runs passes 1 and 2 for l alone -- the same lanes, the same order, hence the same bits of m, l and lse as
//            vtx_attn_map_stats -- and a third pass that stores p_j = __expf(s_j - m) / l (IEEE division) and lse = m + __logf(l).
// P is never written by vtx_attn_map_stats and no buffer of Lq * Lk exists per problem.
//
// vtx_attn_map_meter: one workgroup adds a stats tensor to the fp64 meter [n_layer, nH, 6] in a fixed order (as knn_meter_kernel):
// thread t sums the rows t, t + 256, ... of head h (row = image * Lq + query) in fp64, a halving tree in LDS joins the threads.
//
// vtx_attn_mass_mask: the thresholding of DINO's visualize_attention (sort ascending, cumulative sum, keep what lies above 1 - keep
// of the mass), with these rules.  Values below zero and NaNs count as 0.f.  One workgroup per map sorts the (value, index) pairs
// ascending -- equal values: the lower index first -- by a bitonic network in LDS (4096 pairs of 8 bytes = 32 KB).  THE RUNNING SUM,
// in fp32, in that order, is formed in chunks of 16 consecutive sorted elements, whatever n and the launch geometry:
//     w[c][0] = v[16 c],  w[c][i] = w[c][i - 1] + v[16 c + i]      inside chunk c, left to right
//     P[0] = 0.f,  P[c] = (..((0.f + w[0][15]) + w[1][15]) + ..) + w[c - 1][15]      over the full chunks in front of c, left to right
//     run[16 c + i] = P[c] + w[c][i];     total = run[n - 1];     thr = (1.f - keep) * total   (fp32 subtraction, fp32 product)
// Element e is kept (byte 1) iff run[its sorted position] > thr, else byte 0.  A sum that hits thr exactly is not kept; an all-zero
// map keeps nothing.  DINO's script divides the values by their total before the running sum and compares with 1 - keep; this
// kernel does not divide (one rounding per element less, and an all-zero map has no 0 / 0): the only difference.
//
// WINDOW AND HALO ATTENTION (vtx_attn_mapw_rows / vtx_attn_mapw_stats; template flag WX, every addition behind `if constexpr (WX)`: the
// instantiations above are what they were).  Operands as vtx_attn_hdw_fwd: with win > 0, B images whose packed projection lies in map
// order (H, W); token t of window n of image b is found by the rolled address (am_row = the rule of hd_row), Lq = Lk = win * win,
// problems = B * nW; with win == 0, B problems of plain rows (the gathered q | kv pair of halo attention).  bias fp32 [nH][Lq][Lk] or
// null; mask bytes [nW][Lq][Lk] or null (win > 0 only), nonzero = excluded; every query row keeps at least one unmasked key (the
// precondition of vtx_attn_hdw_fwd).  Term by term (am_scores_w = the cell rule of hdw_add):
//   a_j = acc_j * scale            as above: ONE fp32 multiply, the rounded product settled (acc_settle)
//   s_j = a_j + bias[h][i][j]      with a bias: a SEPARATE fp32 add of the settled product, never one fma with it; the rounded sum is
//                                  settled again and IS the score.  Without a bias s_j = a_j: the same bits as the entries above.
//   excluded cells                 a masked cell and a key >= Lk: never in the maximum (-inf there), e_j = 0 EXACTLY because no
//                                  exponential is formed for it, nothing added to l, es, the self mass or dist: e_j * s_j is skipped,
//                                  not formed, so 0 * -inf never appears.  p of a masked cell is stored as 0.f.
//   passes, lanes, butterfly       as above.  The maximum is final before any exponential is taken, so a key block that is fully masked
//                                  for a query (the rule in shifted windows of more than 64 tokens) needs no -inf - -inf guard: m is
//                                  finite and s_j - m is only formed for cells that count.
//   stats [problems, nH, Lq, 5]    lse = m + __logf(l)    entropy = lse - es / l    smax = m (bias included, masked keys excluded)
//                                  self = e_self / l      dist = ed / l, ed += e_j * v_sqrt_f32((float)(dy^2 + dx^2))
//       window mode: token t sits at (t / win, t % win) of its window, queries and keys alike; self is key j == i.
//       halo mode:   query t sits at (off + t / gq, off + t % gq) of the key grid of width gk, off = (gk - gq) / 2; key j at (j / gk,
//                    j % gk); self is the key at the query's own position.  gq = gk = 0: self and dist store 0.f.
//   With win == 0 and no bias, mask or grids, p, lse and slots 0..2 are the bits of vtx_attn_map_rows / _stats on the same operands.
//   Slot 3 sits where the prefix mass sits: vtx_attn_map_meter with n_prefix = 0 sums [queries, entropy, self, dist, queries, max smax].
//
// WEIGHTED COLUMN SUMS OF P (vtx_attn_map_colsum; new kernels only, the instantiations above are what they were): the primitive of
// attention rollout (a row vector pushed through A_l = residual I + (1 - residual) mean_h P_l) and of the attention a key RECEIVES.
// Operands q, k, ldq, ldkv, B, Lq, Lk, nH, D, dtype exactly as vtx_attn_map_rows; w fp32 [B, R, Lq], 1 <= R <= 16, shared by the heads,
// any finite values, negative ones included.  Term by term:
//   probabilities  s, m, l and p_ij = __expf(s_ij - m_i) / l_i as vtx_attn_map_rows forms them.  Launch 1 (attn_map_ml_kernel) IS passes 1
//                  and 2 of attn_map_rows_kernel -- the same AmRow, the same lanes and order, the same butterfly -- and stores (m_i, l_i)
//                  to the workspace, fp32 [B, nH, Lq, 2].  Launch 2 forms s_ij by am_scores and p_ij by the same expression with the
//                  IEEE division: p_ij is bit for bit the value vtx_attn_map_rows stores.
//   column sums    t = w[b, r, i] * p_ij is ONE fp32 product, rounded on its own, and c[b, h, r, j] the fp32 sum of the t over i: the
//                  product and the add are NEVER contracted into an fma (am_wacc settles the rounded product in a register), so the arithmetic
//                  is the same in every instantiation.  THE ORDER depends on Lq alone.  A workgroup of 4 waves owns one key block of
//                  64 keys of one (image, head) and ALL queries, in tiles of 16 (tile t = queries 16 t .. 16 t + 15, query i in lane
//                  column i % 16):
//                    wave v, per lane and key, from 0.f:   a_v[i % 16] += t_i   over its tiles t = v, v + 4, v + 8, .. ascending
//                    the 16 query lanes meet in one butterfly (group_sum<16>, DPP):   x += x(lane ^ 1);  x += x(lane ^ 2);
//                      x += x(lane ^ 7);  x += x(lane ^ 15)   -- after the first two steps the lanes of a quad hold one value, so
//                      these are the sums of the xor-4 and xor-8 steps; every lane ends with the same bits
//                    the waves meet in LDS in wave order:   c = ((x_0 + x_1) + x_2) + x_3     (a wave without a tile holds 0.f)
//                  Neither B, R, the launch geometry nor the other weight rows of the call enter: a call of more than 4 weight rows
//                  recomputes the scores per chunk of 4 rows, each row's own accumulators apart.  A zero weight contributes an exact
//                  zero (p is finite), so a one-hot row w = e_i gives c[b, h, r, :] = 0.f + .. + 1.f * p_i: + .. + 0.f = the row
//                  p[b, h, i, :] that vtx_attn_map_rows stores, bit for bit (and 2^-3 e_i that row times 2^-3).
//                  c goes to out_heads fp32 [B, nH, R, Lk], or to the workspace when that pointer is null.
//   blend          out_mix fp32 [B, R, Lk] (Lq == Lk), launch 3, one thread per element:
//                    h_sum = (..((c_0 + c_1) + c_2) + ..) + c_{nH - 1}     heads ascending
//                    out_mix[b, r, j] = (alpha * w[b, r, j]) + (beta * h_sum)
//                  two fp32 products and one fp32 sum in that written order, NOT contracted (am_blend settles both products): the envelope
//                  charges one rounding each.  alpha = 1, beta = 0 returns w.
//   bits           an image's outputs do not depend on how the batch is cut into calls, a weight row's not on the other rows of the
//                  call, neither on packed against split operands nor on which of the two outputs are asked for.
// P is never written by vtx_attn_map_colsum and no buffer of Lq * Lk exists per problem: the workspace is (m, l) per query and, without
// out_heads, c: 4 * (2 B nH Lq + B nH R Lk) bytes (vtx_attn_map_colsum_workspace_bytes).
//
// No floating-point atomics anywhere; every sum has a fixed order, so the same inputs give the same bits.
//
// Budget (hipcc resource remarks, gfx950, no scratch in any instantiation): DESIGN.md sections 7i, 7j and 7k.
#include "vtx_common.h"

#define AM_KB 64                 // keys per block (4 tiles of 16)
#define AM_MASK_MAX 4096         // elements of a map at most
#define AM_CHUNK 16              // elements of a chunk of the running sum

struct AmGeom {
  int Lq, Lk, nH, D;
  int qblocks;                   // ceil(nrows / 64)
  int row0, nrows;               // query rows row0 .. row0 + nrows - 1 (stats: 0, Lq)
  int n_prefix, gh, gw;          // stats only; gw == 0: dist off
  int64_t ldq, ldkv;
  float scale;
};

// ---- the window / halo entries (vtx_attn_mapw_*): the same kernels with WX = true take this geometry instead (as HdwGeom extends
// HdGeom in attention_hd.hip).  The existing instantiations (WX = false) see none of it: every addition sits behind `if constexpr (WX)`.
struct AmwGeom : AmGeom {
  const float* bias;             // fp32 [nH][Lq][Lk] or null
  const uint8_t* mask;           // [nW][Lq][Lk] or null; nonzero: the cell is excluded.  Problem (image b, window n) reads mask[n]
  int H, W, win, shift, nWx, nW; // shift = win / 2 or 0; nW = windows per image (1 with win == 0)
  int gq, gk;                    // stats, win == 0: the query grid gq x gq centred in the key grid gk x gk; 0, 0: self and dist off
};
template <bool WX> struct AmG { using type = AmGeom; };
template <> struct AmG<true> { using type = AmwGeom; };

// row of token t of problem p (row0 = p * L: the plain address) -- the rule of hd_row (attention_hd.hip), restated: with win > 0 token t
// of window n of image b is a row of the (H, W) map, the roll by -win / 2 folded into the address
template <bool WX, typename G> __device__ __forceinline__ int64_t am_row(const G& g, int64_t row0, int p, int t) {
  if constexpr (WX) {
    if (g.win) {
      const int b = p / g.nW, n = p - b * g.nW;
      const int wi = n / g.nWx, wj = n - wi * g.nWx;
      const int ay = t / g.win, ax = t - ay * g.win;
      int y = wi * g.win + ay + g.shift; if (y >= g.H) y -= g.H;   // rolled position p holds original (p + win / 2) mod H
      int x = wj * g.win + ax + g.shift; if (x >= g.W) x -= g.W;
      return ((int64_t)b * g.H + y) * g.W + x;
    }
  }
  return row0 + t;
}

template <typename T> __device__ __forceinline__ Vec8<T> am_load(const T* head, int d0, int D, bool valid) {
  const bool in = d0 < D;
  return load8_clamped<T>(head + (in ? d0 : 0), valid && in);
}

// The scaled scores of key block k0 against the wave's query fragments: st[kt][r] = s(query c, key k0 + 16 kt + 4 g + r); keys >= Lk are
// -inf.  The chain of hdattn_fwd_kernel, read in the block of its MFMAs (acc_settle).
template <typename T, int DS>
__device__ __forceinline__ void am_scores(f32x4 (&st)[4], const Vec8<T> (&qf)[DS], const T* __restrict__ kb, int64_t krow0, int64_t ld,
                                          int k0, int Lk, int D, float scale, int c_, int g_) {
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    st[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int key = k0 + kt * 16 + c_;
    const bool kv = key < Lk;
    const T* kp = kb + (krow0 + (kv ? key : 0)) * ld;
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) mma16(am_load<T>(kp, ds * 32 + g_ * 8, D, kv), qf[ds], st[kt]);   // S^T[key][q = c_]
    acc_settle(st[kt]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kk = k0 + kt * 16 + g_ * 4 + r;
      st[kt][r] = kk < Lk ? st[kt][r] * scale : -INFINITY;
    }
    acc_settle(st[kt]);          // the rounded product IS the score: no use of it may be contracted into an fma of acc and scale
  }
}

// (WX) The scores of key block k0 for query token q of problem `prob` (head h, window nwin of its image) under the cell rule of hdw_add
// (attention_hd.hip), restated: a_j = acc_j * scale exactly as above; with a bias s_j = a_j + bias[h][q][j], a SEPARATE fp32 add (the
// rounded product is settled first, so the two are never one fma); a cell whose mask byte is nonzero and a key >= Lk are EXCLUDED: -inf
// in st and a zero bit in the result, bit 4 kt + r = the cell st[kt][r] counts.  Callers test the bit, never the value.
template <typename T, int DS>
__device__ __forceinline__ unsigned am_scores_w(f32x4 (&st)[4], const Vec8<T> (&qf)[DS], const T* __restrict__ kb, const AmwGeom& g, int prob,
                                                int h, int nwin, int q, int k0, int c_, int g_) {
  const int64_t cells = (int64_t)g.Lq * g.Lk, cell0 = (int64_t)q * g.Lk;
  const float* brow = g.bias ? g.bias + h * cells + cell0 : nullptr;
  const uint8_t* mrow = g.mask ? g.mask + nwin * cells + cell0 : nullptr;
  unsigned live = 0;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    st[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int key = k0 + kt * 16 + c_;
    const bool kv = key < g.Lk;
    const T* kp = kb + am_row<true>(g, (int64_t)prob * g.Lk, prob, kv ? key : 0) * g.ldkv;
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) mma16(am_load<T>(kp, ds * 32 + g_ * 8, g.D, kv), qf[ds], st[kt]);   // S^T[key][q = c_]
    acc_settle(st[kt]);
#pragma unroll
    for (int r = 0; r < 4; ++r) st[kt][r] = st[kt][r] * g.scale;
    acc_settle(st[kt]);          // the rounded product, as in am_scores
    const int kb0 = k0 + kt * 16 + g_ * 4;
    if (brow) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (kb0 + r < g.Lk) st[kt][r] += brow[kb0 + r];
      acc_settle(st[kt]);        // the rounded sum IS the score
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kk = kb0 + r;
      bool in = kk < g.Lk;
      if (in && mrow) in = mrow[kk] == 0;
      if (in) live |= 1u << (kt * 4 + r);
      else st[kt][r] = -INFINITY;
    }
  }
  return live;
}

// What every score kernel starts with: the wave's query (row0 + 16 * (4 block + wave) + c), its fragments, pass 1 and pass 2 for l.
template <typename T, int DS, bool WX = false> struct AmRow {
  using G = typename AmG<WX>::type;
  Vec8<T> qf[DS];
  const T* kb;
  int64_t krow0;
  int bh, qi, q, c_, g_;         // qi: index inside the call's rows; q = row0 + qi
  int prob, head, nwin;          // (WX) b = problem, its head, the window of the problem inside its image
  bool qv;
  float m;

  __device__ __forceinline__ void init(const T* __restrict__ qp, const T* __restrict__ kp, const G& g) {
    bh = blockIdx.x / g.qblocks;
    const int qblk = blockIdx.x - bh * g.qblocks;
    const int b = bh / g.nH, h = bh - b * g.nH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    c_ = lane & 15; g_ = lane >> 4;
    qi = (qblk * 4 + wave) * 16 + c_;
    qv = qi < g.nrows;
    q = g.row0 + (qv ? qi : 0);
    const T* qb = qp + h * g.D + am_row<WX>(g, (int64_t)b * g.Lq, b, q) * g.ldq;
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) qf[ds] = am_load<T>(qb, ds * 32 + g_ * 8, g.D, qv);
    kb = kp + h * g.D;
    krow0 = (int64_t)b * g.Lk;
    prob = b; head = h; nwin = 0;
    if constexpr (WX) nwin = b % g.nW;
  }
  __device__ __forceinline__ bool wave_idle(const G& g) const { return qi - c_ >= g.nrows; }   // wave-uniform; no barrier follows
  // -> (WX) the bits of the cells that count (am_scores_w); without WX every key < Lk counts and the result is unused
  __device__ __forceinline__ unsigned scores(f32x4 (&st)[4], int k0, const G& g) const {
    if constexpr (WX) {
      return am_scores_w<T, DS>(st, qf, kb, g, prob, head, nwin, q, k0, c_, g_);
    } else {
      am_scores<T, DS>(st, qf, kb, krow0, g.ldkv, k0, g.Lk, g.D, g.scale, c_, g_);
      return 0u;
    }
  }
  // does cell st[kt][r] = key kk of the block count?  (WX) excluded cells never enter a sum: no e_j is formed for them
  __device__ __forceinline__ bool counts(unsigned live, int kt, int r, int kk, const G& g) const {
    if constexpr (WX) return (live >> (kt * 4 + r)) & 1u;
    else return kk < g.Lk;
  }
  __device__ __forceinline__ void pass_max(const G& g) {
    float mb = -INFINITY;
    for (int k0 = 0; k0 < g.Lk; k0 += AM_KB) {
      f32x4 st[4];
      scores(st, k0, g);
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) mb = fmaxf(mb, st[kt][r]);
    }
    mb = fmaxf(mb, shfl_xor_f(mb, 16));
    m = fmaxf(mb, shfl_xor_f(mb, 32));
  }
};
__device__ __forceinline__ float am_join(float x) {          // the butterfly of a query's four lanes
  x += shfl_xor_f(x, 16);
  x += shfl_xor_f(x, 32);
  return x;
}

// ------------------------------------------------------------------------------------------------- rows of P
// grid = B * nH * ceil(nrows / 64) workgroups of 4 waves; p [B, nH, nrows, Lk], lse [B, nH, nrows]
template <typename T, int DP, bool WX = false>
__global__ __launch_bounds__(256) void attn_map_rows_kernel(const T* __restrict__ qp, const T* __restrict__ kp, float* __restrict__ p,
                                                           float* __restrict__ lse, typename AmG<WX>::type g) {
  constexpr int DS = DP / 32;
  AmRow<T, DS, WX> row;
  row.init(qp, kp, g);
  if (row.wave_idle(g)) return;
  row.pass_max(g);
  const float m = row.m;
  float l = 0.f;
  for (int k0 = 0; k0 < g.Lk; k0 += AM_KB) {
    f32x4 st[4];
    const unsigned live = row.scores(st, k0, g);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (row.counts(live, kt, r, k0 + kt * 16 + row.g_ * 4 + r, g)) l += __expf(st[kt][r] - m);
  }
  l = am_join(l);
  const int64_t orow = (int64_t)row.bh * g.nrows + row.qi;
  if (row.qv && row.g_ == 0) lse[orow] = m + __logf(l);
  for (int k0 = 0; k0 < g.Lk; k0 += AM_KB) {
    f32x4 st[4];
    const unsigned live = row.scores(st, k0, g);
    if (row.qv) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kk = k0 + kt * 16 + row.g_ * 4 + r;
          if constexpr (WX) {
            if (kk < g.Lk) p[orow * g.Lk + kk] = row.counts(live, kt, r, kk, g) ? __expf(st[kt][r] - m) / l : 0.f;   // masked: exactly 0
          } else {
            if (kk < g.Lk) p[orow * g.Lk + kk] = __expf(st[kt][r] - m) / l;
          }
        }
    }
  }
}

// ------------------------------------------------------------------------------------------------- statistics
// grid = B * nH * ceil(Lq / 64); stats [B, nH, Lq, 5] = lse, entropy, smax, prefix, dist
template <typename T, int DP, bool WX = false>
__global__ __launch_bounds__(256) void attn_map_stats_kernel(const T* __restrict__ qp, const T* __restrict__ kp, float* __restrict__ stats,
                                                            typename AmG<WX>::type g) {
  constexpr int DS = DP / 32;
  AmRow<T, DS, WX> row;
  row.init(qp, kp, g);
  if (row.wave_idle(g)) return;
  row.pass_max(g);
  const float m = row.m;
  if constexpr (WX) {
    // window: token t at (t / win, t % win) for queries and keys; halo: query t at (off + t / gq, off + t % gq) of the key grid of width
    // gk, key j at (j / gk, j % gk); kw == 0: no positions, self and dist store 0
    const int kw = g.win ? g.win : g.gk, qw = g.win ? g.win : g.gq;
    const bool on_grid = kw > 0;
    int qy = 0, qx = 0, self = -1;
    if (on_grid) {
      const int off = g.win ? 0 : (g.gk - g.gq) / 2;
      qy = row.q / qw; qx = row.q - qy * qw;
      qy += off; qx += off;
      self = qy * kw + qx;                                            // the key at the query's own position
    }
    float l = 0.f, es = 0.f, ep = 0.f, ed = 0.f;
    for (int k0 = 0; k0 < g.Lk; k0 += AM_KB) {
      f32x4 st[4];
      const unsigned live = row.scores(st, k0, g);
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const int kb0 = k0 + kt * 16 + row.g_ * 4;
        int ky = 0, kx = kb0;
        if (on_grid) { ky = kb0 / kw; kx = kb0 - ky * kw; }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kk = kb0 + r;
          if (row.counts(live, kt, r, kk, g)) {                       // an excluded cell forms no e_j and no e_j * s_j (0 * -inf)
            const float s = st[kt][r];
            const float e = __expf(s - m);
            l += e;
            es += e * s;
            if (on_grid) {
              if (kk == self) ep += e;
              const int dy = ky - qy, dx = kx - qx;
              ed += e * __builtin_amdgcn_sqrtf((float)(dy * dy + dx * dx));
            }
          }
          if (on_grid && ++kx == kw) { kx = 0; ++ky; }
        }
      }
    }
    l = am_join(l);
    es = am_join(es);
    ep = am_join(ep);
    ed = am_join(ed);
    if (row.qv && row.g_ == 0) {
      const float ls = m + __logf(l);
      float* out = stats + ((int64_t)row.bh * g.Lq + row.q) * 5;
      out[0] = ls;
      out[1] = ls - es / l;
      out[2] = m;
      out[3] = on_grid ? ep / l : 0.f;
      out[4] = on_grid ? ed / l : 0.f;
    }
    return;
  }
  // ---- WX = false: the statistics of global attention (prefix tokens, one grid shared by queries and keys), as before
  const int np = g.n_prefix, gw = g.gw;
  const bool on_grid = gw > 0 && row.q >= np;                       // this query has a grid position and dist is on
  int qy = 0, qx = 0;
  if (on_grid) { qy = (row.q - np) / gw; qx = (row.q - np) - qy * gw; }
  float l = 0.f, es = 0.f, ep = 0.f, ed = 0.f;
  for (int k0 = 0; k0 < g.Lk; k0 += AM_KB) {
    f32x4 st[4];
    row.scores(st, k0, g);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const int kb0 = k0 + kt * 16 + row.g_ * 4;
      // grid position of the first patch key of the lane's four: key max(kb0, n_prefix); the next ones step along the row
      const int ts = kb0 > np ? kb0 - np : 0;
      int ky = 0, kx = ts;
      if (on_grid) { ky = ts / gw; kx = ts - ky * gw; }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kk = kb0 + r;
        if (kk < g.Lk) {
          const float s = st[kt][r];
          const float e = __expf(s - m);
          l += e;
          es += e * s;
          if (kk < np) {
            ep += e;
          } else if (on_grid) {
            const int dy = ky - qy, dx = kx - qx;
            ed += e * __builtin_amdgcn_sqrtf((float)(dy * dy + dx * dx));
            if (++kx == gw) { kx = 0; ++ky; }
          }
        }
      }
    }
  }
  l = am_join(l);
  es = am_join(es);
  ep = am_join(ep);
  ed = am_join(ed);
  if (row.qv && row.g_ == 0) {
    const float ls = m + __logf(l);
    float* out = stats + ((int64_t)row.bh * g.Lq + row.q) * 5;
    out[0] = ls;
    out[1] = ls - es / l;
    out[2] = m;
    out[3] = ep / l;
    out[4] = on_grid ? ed / l : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------- meter
// meter[layer][h] = [queries, sum entropy, sum prefix, sum dist over patch queries, patch queries, max smax]
__global__ __launch_bounds__(256) void attn_map_meter_kernel(const float* __restrict__ stats, double* __restrict__ meter, int layer, int B,
                                                            int nH, int Lq, int n_prefix) {
  __shared__ double red[4][256];
  const int tid = threadIdx.x;
  const int64_t rows = (int64_t)B * Lq;
  for (int h = 0; h < nH; ++h) {
    double se = 0.0, sp = 0.0, sd = 0.0, mx = -INFINITY;
    for (int64_t i = tid; i < rows; i += 256) {
      const int64_t b = i / Lq;
      const int q = (int)(i - b * Lq);
      const float* s = stats + ((b * nH + h) * Lq + q) * 5;
      se += (double)s[1];
      sp += (double)s[3];
      if (q >= n_prefix) sd += (double)s[4];
      mx = fmax(mx, (double)s[2]);
    }
    red[0][tid] = se; red[1][tid] = sp; red[2][tid] = sd; red[3][tid] = mx;
    __syncthreads();
    for (int sft = 128; sft >= 1; sft >>= 1) {
      if (tid < sft) {
        red[0][tid] += red[0][tid + sft]; red[1][tid] += red[1][tid + sft]; red[2][tid] += red[2][tid + sft];
        red[3][tid] = fmax(red[3][tid], red[3][tid + sft]);
      }
      __syncthreads();
    }
    if (tid == 0) {
      double* o = meter + ((int64_t)layer * nH + h) * 6;
      o[0] += (double)rows; o[1] += red[0][0]; o[2] += red[1][0]; o[3] += red[2][0];
      o[4] += (double)B * (double)(Lq - n_prefix);
      o[5] = fmax(o[5], red[3][0]);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------- mass mask
// one workgroup per map; n2 = the power of two >= max(n, 2)
__global__ __launch_bounds__(256) void attn_mass_mask_kernel(const float* __restrict__ maps, uint8_t* __restrict__ mask, int n, int n2,
                                                            float keep) {
  __shared__ unsigned long long srt[AM_MASK_MAX];             // (value bits << 32) | index: non-negative floats order as their bits
  __shared__ float tot[AM_MASK_MAX / AM_CHUNK];
  __shared__ float total_s;
  const int tid = threadIdx.x;
  const float* src = maps + (int64_t)blockIdx.x * n;
  uint8_t* dst = mask + (int64_t)blockIdx.x * n;
  for (int i = tid; i < n2; i += 256) {
    unsigned long long kv = ~0ull;                             // the pad sorts behind every element
    if (i < n) kv = ((unsigned long long)__float_as_uint(fmaxf(src[i], 0.f)) << 32) | (unsigned)i;   // below zero, NaN, -0.f: +0.f
    srt[i] = kv;
  }
  __syncthreads();
  for (int size = 2; size <= n2; size <<= 1)
    for (int stride = size >> 1; stride >= 1; stride >>= 1) {
      for (int t = tid; t < (n2 >> 1); t += 256) {
        const int lo = ((t / stride) * stride << 1) + (t % stride), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const unsigned long long a = srt[lo], b = srt[hi];
        if ((a > b) == up) { srt[lo] = b; srt[hi] = a; }
      }
      __syncthreads();
    }
  // chunk c of 16 sorted elements belongs to thread c (n <= 4096 = 256 * 16)
  const int e0 = tid * AM_CHUNK;
  float w[AM_CHUNK];
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < AM_CHUNK; ++i) {
    const float v = e0 + i < n ? __uint_as_float((unsigned)(srt[e0 + i] >> 32)) : 0.f;
    acc = i == 0 ? v : acc + v;
    w[i] = acc;
  }
  tot[tid] = acc;
  __syncthreads();
  float P = 0.f;
  for (int c = 0; c < tid && c * AM_CHUNK < n; ++c) P += tot[c];
#pragma unroll
  for (int i = 0; i < AM_CHUNK; ++i) w[i] = P + w[i];
  if (e0 <= n - 1 && n - 1 < e0 + AM_CHUNK) {
    float last = w[0];
#pragma unroll
    for (int i = 1; i < AM_CHUNK; ++i)
      if (e0 + i == n - 1) last = w[i];
    total_s = last;
  }
  __syncthreads();
  const float thr = (1.f - keep) * total_s;
#pragma unroll
  for (int i = 0; i < AM_CHUNK; ++i)
    if (e0 + i < n) dst[(unsigned)(srt[e0 + i] & 0xffffffffull)] = w[i] > thr ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------- weighted column sums of P
#define AM_RMAX 16               // weight rows of a call at most
#define AM_RC 4                  // weight rows per chunk: 16 accumulators each, the scores recomputed per chunk

// One product and one sum, each rounded on its own: never an fma, whatever the instantiation around it (WEIGHTED COLUMN SUMS).  The build
// contracts wherever it can (-ffp-contract=fast), so the rounded product is settled in a register before the add, as acc_settle does.
__device__ __forceinline__ float am_settle(float t) { asm volatile("" : "+v"(t)); return t; }
__device__ __forceinline__ float am_wacc(float acc, float w, float p) { return acc + am_settle(w * p); }
// out_mix = (alpha * w) + (beta * h_sum): two rounded products and a sum in that order, not contracted.
__device__ __forceinline__ float am_blend(float alpha, float w, float beta, float hsum) {
  return am_settle(alpha * w) + am_settle(beta * hsum);
}

// launch 1: passes 1 and 2 of attn_map_rows_kernel for all Lq rows (g.row0 = 0, g.nrows = Lq); ml [B, nH, Lq, 2] = (m, l).
// grid = B * nH * ceil(Lq / 64)
template <typename T, int DP>
__global__ __launch_bounds__(256) void attn_map_ml_kernel(const T* __restrict__ qp, const T* __restrict__ kp, float* __restrict__ ml,
                                                         AmGeom g) {
  constexpr int DS = DP / 32;
  AmRow<T, DS> row;
  row.init(qp, kp, g);
  if (row.wave_idle(g)) return;
  row.pass_max(g);
  const float m = row.m;
  float l = 0.f;
  for (int k0 = 0; k0 < g.Lk; k0 += AM_KB) {
    f32x4 st[4];
    const unsigned live = row.scores(st, k0, g);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (row.counts(live, kt, r, k0 + kt * 16 + row.g_ * 4 + r, g)) l += __expf(st[kt][r] - m);
  }
  l = am_join(l);
  if (row.qv && row.g_ == 0) {
    float* o = ml + ((int64_t)row.bh * g.Lq + row.qi) * 2;
    o[0] = m;
    o[1] = l;
  }
}

// launch 2: grid = B * nH * kblocks (kblocks = ceil(Lk / 64)); a workgroup owns key block k0 .. k0 + 63 of (image b, head h) and every
// query; c [B, nH, R, Lk].  RC = weight rows per chunk (1: the single row of a CLS rollout; AM_RC otherwise).
template <typename T, int DP, int RC>
__global__ __launch_bounds__(256) void attn_map_colsum_kernel(const T* __restrict__ qp, const T* __restrict__ kp,
                                                             const float* __restrict__ ml, const float* __restrict__ w,
                                                             float* __restrict__ c, AmGeom g, int R, int kblocks) {
  constexpr int DS = DP / 32;
  __shared__ float red[4][RC][AM_KB];
  const int bh = blockIdx.x / kblocks;
  const int k0 = (blockIdx.x - bh * kblocks) * AM_KB;
  const int b = bh / g.nH, h = bh - b * g.nH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c_ = lane & 15, g_ = lane >> 4;
  const T* qb = qp + h * g.D;
  const T* kb = kp + h * g.D;
  const int64_t qrow0 = (int64_t)b * g.Lq, krow0 = (int64_t)b * g.Lk;
  const float* mlb = ml + (int64_t)bh * g.Lq * 2;
  const int ntiles = (g.Lq + 15) / 16;
  for (int r0 = 0; r0 < R; r0 += RC) {
    f32x4 acc[RC][4];
#pragma unroll
    for (int rr = 0; rr < RC; ++rr)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) acc[rr][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = wave; t < ntiles; t += 4) {                          // wave-uniform: the MFMAs run with every lane
      const int q = t * 16 + c_;
      const bool qv = q < g.Lq;
      const T* qrow = qb + (qrow0 + (qv ? q : 0)) * g.ldq;
      Vec8<T> qf[DS];
#pragma unroll
      for (int ds = 0; ds < DS; ++ds) qf[ds] = am_load<T>(qrow, ds * 32 + g_ * 8, g.D, qv);
      float m = 0.f, l = 1.f, wq[RC];
      if (qv) { m = mlb[2 * q]; l = mlb[2 * q + 1]; }
#pragma unroll
      for (int rr = 0; rr < RC; ++rr) wq[rr] = (qv && r0 + rr < R) ? w[((int64_t)b * R + r0 + rr) * g.Lq + q] : 0.f;
      f32x4 st[4];
      am_scores<T, DS>(st, qf, kb, krow0, g.ldkv, k0, g.Lk, g.D, g.scale, c_, g_);
      if (qv) {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (k0 + kt * 16 + g_ * 4 + r < g.Lk) {
              const float p = __expf(st[kt][r] - m) / l;               // the expression of attn_map_rows_kernel
#pragma unroll
              for (int rr = 0; rr < RC; ++rr) acc[rr][kt][r] = am_wacc(acc[rr][kt][r], wq[rr], p);
            }
      }
    }
#pragma unroll
    for (int rr = 0; rr < RC; ++rr)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float x = group_sum<16>(acc[rr][kt][r]);                     // the butterfly of a key's 16 query lanes (DPP)
          vmem_guard(x);                                               // LDS store data: one wait state behind packed math
          if (c_ == 0) red[wave][rr][kt * 16 + g_ * 4 + r] = x;
        }
    __syncthreads();
    for (int i = threadIdx.x; i < RC * AM_KB; i += 256) {
      const int rr = i / AM_KB, j = i - rr * AM_KB;
      if (r0 + rr < R && k0 + j < g.Lk) {
        float s = red[0][rr][j];                                       // the waves in wave order
        s += red[1][rr][j];
        s += red[2][rr][j];
        s += red[3][rr][j];
        c[((int64_t)bh * R + r0 + rr) * g.Lk + k0 + j] = s;
      }
    }
    __syncthreads();
  }
}

// launch 3: out [B, R, L] = (alpha * w) + (beta * sum_h c[b, h, r, j]), heads ascending; one thread per element
__global__ __launch_bounds__(256) void attn_map_mix_kernel(const float* __restrict__ c, const float* __restrict__ w, float* __restrict__ out,
                                                          float alpha, float beta, int64_t n, int nH, int R, int L) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t rl = (int64_t)R * L;
  const int64_t b = i / rl, rj = i - b * rl;
  const float* cp = c + b * nH * rl + rj;
  float s = cp[0];
  for (int h = 1; h < nH; ++h) s += cp[h * rl];
  out[i] = am_blend(alpha, w[i], beta, s);
}

// ------------------------------------------------------------------------------------------------- host
template <typename T, int DP> static int am_ml_t(const void* q, const void* k, float* ml, int B, const AmGeom& g, hipStream_t st) {
  hipLaunchKernelGGL((attn_map_ml_kernel<T, DP>), dim3((unsigned)(B * g.nH * g.qblocks)), dim3(256), 0, st, (const T*)q, (const T*)k, ml, g);
  return vtx_check_launch();
}
template <typename T, int DP> static int am_colsum_t(const void* q, const void* k, const float* ml, const float* w, float* c, int B, int R,
                                                     int kblocks, const AmGeom& g, hipStream_t st) {
  const dim3 grid((unsigned)(B * g.nH * kblocks));
  if (R == 1)
    hipLaunchKernelGGL((attn_map_colsum_kernel<T, DP, 1>), grid, dim3(256), 0, st, (const T*)q, (const T*)k, ml, w, c, g, R, kblocks);
  else
    hipLaunchKernelGGL((attn_map_colsum_kernel<T, DP, AM_RC>), grid, dim3(256), 0, st, (const T*)q, (const T*)k, ml, w, c, g, R, kblocks);
  return vtx_check_launch();
}
template <typename T, int DP> static int am_rows_t(const void* q, const void* k, float* p, float* lse, int B, const AmGeom& g, hipStream_t st) {
  hipLaunchKernelGGL((attn_map_rows_kernel<T, DP>), dim3((unsigned)(B * g.nH * g.qblocks)), dim3(256), 0, st, (const T*)q, (const T*)k, p,
                     lse, g);
  return vtx_check_launch();
}
template <typename T, int DP> static int am_stats_t(const void* q, const void* k, float* stats, int B, const AmGeom& g, hipStream_t st) {
  hipLaunchKernelGGL((attn_map_stats_kernel<T, DP>), dim3((unsigned)(B * g.nH * g.qblocks)), dim3(256), 0, st, (const T*)q, (const T*)k,
                     stats, g);
  return vtx_check_launch();
}
#define AM_DISPATCH_T(FN, T, ...)                                                                     \
  (D <= 32 ? FN<T, 32>(__VA_ARGS__) : D <= 64 ? FN<T, 64>(__VA_ARGS__) : D <= 96 ? FN<T, 96>(__VA_ARGS__) : FN<T, 128>(__VA_ARGS__))
#define AM_DISPATCH(FN, ...) (dtype == VTX_BF16 ? AM_DISPATCH_T(FN, bf16, __VA_ARGS__) : AM_DISPATCH_T(FN, float, __VA_ARGS__))

// Everything the two score entries refuse, before any launch, with the codes of the vtx_attn_hd_* entries.
static int am_geom(AmGeom& g, int B, int Lq, int Lk, int nH, int D, int row0, int nrows, int dtype, int64_t ldq, int64_t ldkv) {
  if (dtype != VTX_BF16 && dtype != VTX_F32) return VTX_ERR_DTYPE;
  if (B <= 0 || Lq <= 0 || Lk <= 0 || nH <= 0 || D < 8 || D > 128 || D % 8 != 0) return VTX_ERR_SHAPE;
  if ((int64_t)B * Lq >= 0x7fffffffLL || (int64_t)B * Lk >= 0x7fffffffLL || (int64_t)nH * D >= 0x7fffffffLL) return VTX_ERR_SHAPE;
  if (row0 < 0 || nrows <= 0 || (int64_t)row0 + nrows > Lq) return VTX_ERR_SHAPE;
  const int64_t hd = (int64_t)nH * D;
  if (ldq < hd || ldkv < hd) return VTX_ERR_SHAPE;
  if (ldq % 8 || ldkv % 8) return VTX_ERR_ALIGN;
  const int qblocks = (nrows + AM_KB - 1) / AM_KB;
  if ((int64_t)B * nH * qblocks >= 0x7fffffffLL) return VTX_ERR_SHAPE;
  g = AmGeom{Lq, Lk, nH, D, qblocks, row0, nrows, 0, 0, 0, ldq, ldkv, 1.0f / sqrtf((float)D)};
  return VTX_OK;
}
static bool am_aligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) == 0; }

// ---- the window / halo entries
template <typename T, int DP> static int amw_rows_t(const void* q, const void* k, float* p, float* lse, int nprob, const AmwGeom& g, hipStream_t st) {
  hipLaunchKernelGGL((attn_map_rows_kernel<T, DP, true>), dim3((unsigned)(nprob * g.nH * g.qblocks)), dim3(256), 0, st, (const T*)q,
                     (const T*)k, p, lse, g);
  return vtx_check_launch();
}
template <typename T, int DP> static int amw_stats_t(const void* q, const void* k, float* stats, int nprob, const AmwGeom& g, hipStream_t st) {
  hipLaunchKernelGGL((attn_map_stats_kernel<T, DP, true>), dim3((unsigned)(nprob * g.nH * g.qblocks)), dim3(256), 0, st, (const T*)q,
                     (const T*)k, stats, g);
  return vtx_check_launch();
}
// Everything the two window / halo entries refuse, before any launch, with the codes of hdw_geom (attention_hd.hip) and am_geom;
// nprob = the problems of the call: B with win == 0, B * windows per image with win > 0.
static int amw_geom(AmwGeom& g, int64_t& nprob, const float* bias, const uint8_t* mask, int B, int Lq, int Lk, int nH, int D, int H, int W,
                    int win, int shift, int row0, int nrows, int dtype, int64_t ldq, int64_t ldkv) {
  if (dtype != VTX_BF16 && dtype != VTX_F32) return VTX_ERR_DTYPE;
  if (B <= 0 || Lq <= 0 || Lk <= 0 || win < 0) return VTX_ERR_SHAPE;
  nprob = B;
  if (win > 0) {
    if (H <= 0 || W <= 0 || H % win || W % win || (int64_t)win * win != Lq || Lq != Lk) return VTX_ERR_SHAPE;
    nprob = (int64_t)B * (H / win) * (W / win);
  } else if (mask != nullptr) {
    return VTX_ERR_SHAPE;                                           // the mask is per window
  }
  if (nprob >= 0x7fffffffLL) return VTX_ERR_SHAPE;
  AmGeom base;
  int rc = am_geom(base, (int)nprob, Lq, Lk, nH, D, row0, nrows, dtype, ldq, ldkv);
  if (rc) return rc;
  if ((int64_t)nH * Lq * Lk >= 0x7fffffffLL) return VTX_ERR_SHAPE;
  static_cast<AmGeom&>(g) = base;
  g.bias = bias; g.mask = mask;
  g.H = H; g.W = W; g.win = win; g.shift = (win && shift) ? win / 2 : 0;
  g.nWx = win ? W / win : 1; g.nW = win ? (H / win) * (W / win) : 1;
  g.gq = 0; g.gk = 0;
  return VTX_OK;
}

extern "C" {

/* include/vtx.h: vtx_attn_map_rows */
int vtx_attn_map_rows(const void* q, const void* k, int64_t ldq, int64_t ldkv, float* p, float* lse, int B, int Lq, int Lk, int nH, int D,
                      int row0, int nrows, int dtype, void* stream) {
  if (!q || !k || !p || !lse) return VTX_ERR_NULL;
  AmGeom g;
  int rc = am_geom(g, B, Lq, Lk, nH, D, row0, nrows, dtype, ldq, ldkv);
  if (rc) return rc;
  if (!am_aligned(q, 15) || !am_aligned(k, 15) || !am_aligned(p, 3) || !am_aligned(lse, 3)) return VTX_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  return AM_DISPATCH(am_rows_t, q, k, p, lse, B, g, st);
}

/* include/vtx.h: vtx_attn_map_stats */
int vtx_attn_map_stats(const void* q, const void* k, int64_t ldq, int64_t ldkv, float* stats, int B, int Lq, int Lk, int nH, int D,
                       int n_prefix, int gh, int gw, int dtype, void* stream) {
  if (!q || !k || !stats) return VTX_ERR_NULL;
  AmGeom g;
  int rc = am_geom(g, B, Lq, Lk, nH, D, 0, Lq > 0 ? Lq : 1, dtype, ldq, ldkv);
  if (rc) return rc;
  if (n_prefix < 0 || n_prefix > (Lq < Lk ? Lq : Lk)) return VTX_ERR_SHAPE;
  if (gh != 0 || gw != 0) {          // keys and queries share one grid
    if (gh <= 0 || gw <= 0 || (int64_t)gh * gw != (int64_t)Lk - n_prefix || (int64_t)gh * gw != (int64_t)Lq - n_prefix) return VTX_ERR_SHAPE;
  }
  if (!am_aligned(q, 15) || !am_aligned(k, 15) || !am_aligned(stats, 3)) return VTX_ERR_ALIGN;
  g.n_prefix = n_prefix; g.gh = gh; g.gw = gw;
  hipStream_t st = (hipStream_t)stream;
  return AM_DISPATCH(am_stats_t, q, k, stats, B, g, st);
}

/* include/vtx.h: vtx_attn_mapw_rows */
int vtx_attn_mapw_rows(const void* q, const void* k, int64_t ldq, int64_t ldkv, float* p, float* lse, const float* bias,
                       const uint8_t* mask, int B, int Lq, int Lk, int nH, int D, int H, int W, int win, int shift, int row0, int nrows,
                       int dtype, void* stream) {
  if (!q || !k || !p || !lse) return VTX_ERR_NULL;
  AmwGeom g;
  int64_t nprob;
  int rc = amw_geom(g, nprob, bias, mask, B, Lq, Lk, nH, D, H, W, win, shift, row0, nrows, dtype, ldq, ldkv);
  if (rc) return rc;
  if (!am_aligned(q, 15) || !am_aligned(k, 15) || !am_aligned(p, 3) || !am_aligned(lse, 3) || !am_aligned(bias, 3)) return VTX_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  return AM_DISPATCH(amw_rows_t, q, k, p, lse, (int)nprob, g, st);
}

/* include/vtx.h: vtx_attn_mapw_stats */
int vtx_attn_mapw_stats(const void* q, const void* k, int64_t ldq, int64_t ldkv, float* stats, const float* bias, const uint8_t* mask,
                        int B, int Lq, int Lk, int nH, int D, int H, int W, int win, int shift, int gq, int gk, int dtype, void* stream) {
  if (!q || !k || !stats) return VTX_ERR_NULL;
  AmwGeom g;
  int64_t nprob;
  int rc = amw_geom(g, nprob, bias, mask, B, Lq, Lk, nH, D, H, W, win, shift, 0, Lq > 0 ? Lq : 1, dtype, ldq, ldkv);
  if (rc) return rc;
  if (win == 0 && (gq != 0 || gk != 0)) {       // the query grid gq x gq sits centred in the key grid gk x gk
    if (gq <= 0 || gk < gq || (int64_t)gq * gq != Lq || (int64_t)gk * gk != Lk || (gk - gq) % 2) return VTX_ERR_SHAPE;
    g.gq = gq; g.gk = gk;
  }
  if (!am_aligned(q, 15) || !am_aligned(k, 15) || !am_aligned(stats, 3) || !am_aligned(bias, 3)) return VTX_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  return AM_DISPATCH(amw_stats_t, q, k, stats, (int)nprob, g, st);
}

/* include/vtx.h: vtx_attn_map_colsum_workspace_bytes -- (m, l) per query and room for c [B, nH, R, Lk]; 0 for sizes the entry refuses */
size_t vtx_attn_map_colsum_workspace_bytes(int B, int Lq, int Lk, int nH, int R) {
  if (B <= 0 || Lq <= 0 || Lk <= 0 || nH <= 0 || R < 1 || R > AM_RMAX) return 0;
  return ((size_t)2 * B * nH * Lq + (size_t)B * nH * R * Lk) * sizeof(float);
}

/* include/vtx.h: vtx_attn_map_colsum */
int vtx_attn_map_colsum(const void* q, const void* k, int64_t ldq, int64_t ldkv, const float* w, float* out_heads, float* out_mix,
                        float alpha, float beta, int B, int Lq, int Lk, int nH, int D, int R, void* ws, size_t ws_bytes, int dtype,
                        void* stream) {
  if (!q || !k || !w || (!out_heads && !out_mix)) return VTX_ERR_NULL;
  AmGeom g;
  int rc = am_geom(g, B, Lq, Lk, nH, D, 0, Lq > 0 ? Lq : 1, dtype, ldq, ldkv);
  if (rc) return rc;
  if (R < 1 || R > AM_RMAX) return VTX_ERR_SHAPE;
  if (out_mix && Lq != Lk) return VTX_ERR_SHAPE;
  if (!(fabsf(alpha) <= 3.402823466e+38f) || !(fabsf(beta) <= 3.402823466e+38f)) return VTX_ERR_SHAPE;   // NaN, inf
  const int kblocks = (Lk + AM_KB - 1) / AM_KB;
  if ((int64_t)B * nH * kblocks >= 0x7fffffffLL) return VTX_ERR_SHAPE;
  if (!am_aligned(q, 15) || !am_aligned(k, 15) || !am_aligned(w, 3) || !am_aligned(out_heads, 3) || !am_aligned(out_mix, 3) ||
      !am_aligned(ws, 3))
    return VTX_ERR_ALIGN;
  if (!ws || ws_bytes < vtx_attn_map_colsum_workspace_bytes(B, Lq, Lk, nH, R)) return VTX_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* ml = (float*)ws;
  float* c = out_heads ? out_heads : ml + (size_t)2 * B * nH * Lq;
  rc = AM_DISPATCH(am_ml_t, q, k, ml, B, g, st);
  if (rc) return rc;
  rc = AM_DISPATCH(am_colsum_t, q, k, ml, w, c, B, R, kblocks, g, st);
  if (rc || !out_mix) return rc;
  const int64_t n = (int64_t)B * R * Lk;
  hipLaunchKernelGGL(attn_map_mix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, c, w, out_mix, alpha, beta, n, nH, R, Lk);
  return vtx_check_launch();
}

/* include/vtx.h: vtx_attn_map_meter */
int vtx_attn_map_meter(const float* stats, double* meter, int layer, int B, int nH, int Lq, int n_prefix, void* stream) {
  if (!stats || !meter) return VTX_ERR_NULL;
  if (layer < 0 || B <= 0 || nH <= 0 || Lq <= 0 || n_prefix < 0 || n_prefix > Lq) return VTX_ERR_SHAPE;
  if ((int64_t)B * Lq >= 0x7fffffffLL || (int64_t)layer * nH >= 0x7fffffffLL) return VTX_ERR_SHAPE;
  if (!am_aligned(stats, 3) || !am_aligned(meter, 7)) return VTX_ERR_ALIGN;
  hipLaunchKernelGGL(attn_map_meter_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, stats, meter, layer, B, nH, Lq, n_prefix);
  return vtx_check_launch();
}

/* include/vtx.h: vtx_attn_mass_mask */
int vtx_attn_mass_mask(const float* maps, uint8_t* mask, int n_maps, int n, float keep, void* stream) {
  if (!maps || !mask) return VTX_ERR_NULL;
  if (n_maps <= 0 || n <= 0 || n > AM_MASK_MAX) return VTX_ERR_SHAPE;
  if (!(keep > 0.f) || !(keep <= 1.f)) return VTX_ERR_SHAPE;
  if (!am_aligned(maps, 3)) return VTX_ERR_ALIGN;
  int n2 = 2;
  while (n2 < n) n2 <<= 1;
  hipLaunchKernelGGL(attn_mass_mask_kernel, dim3((unsigned)n_maps), dim3(256), 0, (hipStream_t)stream, maps, mask, n, n2, keep);
  return vtx_check_launch();
}

}  // extern "C"
