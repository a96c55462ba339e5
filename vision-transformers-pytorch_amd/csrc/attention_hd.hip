// Global attention for ANY head width D that is a multiple of 8 up to 128 (ViT-H/14: 80; 12-head ViT-S: 32; CaiT: 48; PVT widths that
// are not 64 x heads) and any number of queries and keys: the widths the register-resident kernels (attention.hip, attention_seq.hip,
// attention_sr.hip) and the key-block kernels of attention_long.hip (D = 64 | 32) do not serve.  The reference's modules take any
// dim // n_head (models/vit.py:20, pvt.py:12-30, twins.py:39-93).
//
// softmax(q k^T / sqrt(D)) v for queries [B * Lq, nH * D] (row stride ldq) against keys / values [B * Lk, nH * D] (row stride ldkv),
// given by three pointers: the packed QKV projection (Lq = Lk, ldq = ldkv = 3 nH D) or the q | kv pair of the sub-sampled attention
// (ldq = nH D, ldkv = 2 nH D).  No bias, no mask in vtx_attn_hd_*; window and halo attention (Swin, the Twins locally-grouped half,
// Halo: swin_transformer.py:25-40, twins.py:109-157, halo_transformer.py:23-30) take the same kernels with an additive score bias, a
// byte mask and window addressing (template flag WX, vtx_attn_hdw_*, below).
//
// The arithmetic is attention_long.hip's: keys in blocks of 64 with an online softmax, P packed to the operand type for P V, the
// backward in two launches (dQ per query tile over all key blocks; dK / dV per key tile over all query blocks) with P recomputed
// from the saved log-sum-exp; every output element is owned by one wave (deterministic, no atomics).
//
// PADDING RULE.  The kernels are templated on the padded width DP in {32, 64, 96, 128}; the true D is a runtime number.  Every operand
// moves in 8-element vectors and D % 8 == 0, so the pad is whole vectors.  A vector that starts at d0 >= D is a ZERO operand and its
// memory is never touched: the fragment loads (hd_load) clamp d0 to 0 -- the first vector of the same head of the same row, always
// inside the row -- and discard what they read (a select, no branch: see load8_clamped); the staging loop (hd_stage_t) predicates the
// load.  Without this the last head of the last row would read up to (DP - D) elements past the allocation.  Output and gradient
// columns >= D are never stored.
//
// Budget per DP (bf16 | fp32), 256 threads: LDS of the forward / dQ kernel = DP * 72 elements (4.5 | 9, 9 | 18, 13.5 | 27, 18 | 36 KB), of
// the dK / dV kernel twice that + 512 B; accumulators DP / 4 fp32 registers per lane (dK / dV: DP / 2), the wave's own operand fragments
// DP / 8 | DP / 4 registers (dQ, dK / dV: twice that).
#include "vtx_common.h"

#define HD_KB 64                 // tokens per block (4 tiles of 16)
#define HD_STR (HD_KB + 8)       // transposed LDS row stride

struct HdGeom {
  int Lq, Lk, nH, D, hd;         // hd = nH * D: the row stride of o / dout
  int qblocks, kblocks;          // ceil(Lq / 64), ceil(Lk / 64)
  int64_t ldq, ldkv, lddq, lddkv;
  float scale;
  DropArgs drop;                 // drop.scale == 0: off.  problem = image * nH + head
};
__device__ __forceinline__ float hd_drop(const HdGeom& g, int bh, int q, int key) {
  return g.drop.scale == 0.f ? 1.f : drop_factor(g.drop, (unsigned)bh, q, key);
}

// ---- the window / halo entries (vtx_attn_hdw_*): the same kernels with WX = true take this geometry instead.  An additive fp32 score bias
// [nH][Lq][Lk], a byte mask [nW][Lq][Lk] (nonzero: the score is -inf; problem (image b, window n) reads mask[n]) and window addressing:
// with win > 0 token t of window n of image b is a row of the (H, W) NHWC map, the roll by -win/2 and back folded into the address
// (what vtx_attention_fwd does with swin != 0), for q, k, v, o, dout and every gradient alike; win == 0: plain rows problem * L + t.
// The existing instantiations (WX = false) see none of this: every addition sits behind `if constexpr (WX)`.
struct HdwGeom : HdGeom {
  const float* bias;
  const uint8_t* mask;
  int H, W, win, shift, nWx, nW;   // shift = win / 2 or 0; nW = windows per image (1 with win == 0)
};
template <bool WX> struct HdG { using type = HdGeom; };
template <> struct HdG<true> { using type = HdwGeom; };

// row of token t of problem p (row0 = p * L: the plain address)
template <bool WX, typename G> __device__ __forceinline__ int64_t hd_row(const G& g, int64_t row0, int p, int t) {
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
// bias + mask term of score (q, key) of head h in window n (q < Lq, key < Lk): -inf for a masked cell
__device__ __forceinline__ float hdw_add(const HdwGeom& g, int h, int n, int q, int key) {
  const int64_t cell = (int64_t)q * g.Lk + key, cells = (int64_t)g.Lq * g.Lk;
  float v = g.bias ? g.bias[h * cells + cell] : 0.f;
  if (g.mask && g.mask[n * cells + cell]) v = -INFINITY;
  return v;
}

// 8 elements at column d0 of a head whose first element is `head` (a readable row: the caller clamps the token).  d0 >= D: the
// address is clamped to the head's first vector and the result is zeros -- nothing beyond the head's D columns is read.
template <typename T> __device__ __forceinline__ Vec8<T> hd_load(const T* head, int d0, int D, bool valid) {
  const bool in = d0 < D;
  return load8_clamped<T>(head + (in ? d0 : 0), valid && in);
}
template <typename T> __device__ __forceinline__ Vec8<T> hd_frag_acc(const f32x4& lo, const f32x4& hi) {
  Vec8<T> f;
#pragma unroll
  for (int j = 0; j < 4; ++j) { f.set(j, lo[j]); f.set(4 + j, hi[j]); }
  return f;
}
template <typename T> __device__ __forceinline__ Vec8<T> hd_frag_t(const T* p, int g) {   // p -> Xt[d][32 * ks]
  Vec8<T> f;
  if constexpr (sizeof(T) == 2) {
    bf16x4 a = *reinterpret_cast<const bf16x4*>(p + 4 * g);
    bf16x4 b = *reinterpret_cast<const bf16x4*>(p + 16 + 4 * g);
#pragma unroll
    for (int j = 0; j < 4; ++j) { f.v[j] = a[j]; f.v[4 + j] = b[j]; }
  } else {
    f32x4 a = *reinterpret_cast<const f32x4*>(p + 4 * g);
    f32x4 b = *reinterpret_cast<const f32x4*>(p + 16 + 4 * g);
#pragma unroll
    for (int j = 0; j < 4; ++j) { f.v[j] = a[j]; f.v[4 + j] = b[j]; }
  }
  return f;
}
// X[tok0 .. tok0 + 64)[0..D) of one head (src = the head's first element in row 0 of the tensor, row stride ld) -> Xt[d][HD_STR];
// tokens >= L and columns >= D are zeros that are never loaded
template <typename T, int DP, bool WX = false, typename G = HdGeom>
__device__ __forceinline__ void hd_stage_t(T* __restrict__ xt, const T* __restrict__ src, int64_t ld, int64_t row0, int tok0, int L,
                                           int D, const G& g = G{}, int p = 0) {
  constexpr int DV = DP / 8;
  for (int idx = threadIdx.x; idx < HD_KB * DV; idx += blockDim.x) {
    const int t = idx / DV, dv = idx - t * DV;
    Vec8<T> v = vec8_zero<T>();
    if constexpr (WX) {
      if (tok0 + t < L && dv * 8 < D) v = load8<T>(src + hd_row<true>(g, row0, p, tok0 + t) * ld + dv * 8);
    } else {
      if (tok0 + t < L && dv * 8 < D) v = load8<T>(src + (row0 + tok0 + t) * ld + dv * 8);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) xt[(dv * 8 + e) * HD_STR + t] = v.v[e];
  }
}

// ------------------------------------------------------------------------------------------------- forward
// grid = B * nH * ceil(Lq / 64) (query block fastest); wave w of a block owns query tile 4 * block + w
template <typename T, int DP, bool WX = false>
__global__ __launch_bounds__(256) void hdattn_fwd_kernel(const T* __restrict__ qp, const T* __restrict__ kp_, const T* __restrict__ vp,
                                                        T* __restrict__ o, float* __restrict__ lse, typename HdG<WX>::type g) {
  constexpr int DS = DP / 32, DT = DP / 16;
  __shared__ __attribute__((aligned(16))) T vt[DP * HD_STR];
  const int bh = blockIdx.x / g.qblocks, qblk = blockIdx.x - bh * g.qblocks;
  const int b = bh / g.nH, h = bh - b * g.nH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c_ = lane & 15, g_ = lane >> 4;
  const int D = g.D;
  const int64_t ldq = g.ldq, ld = g.ldkv, qrow0 = (int64_t)b * g.Lq, row0 = (int64_t)b * g.Lk;
  const T* qb = qp + h * D;
  const T* kb = kp_ + h * D;
  const T* vb = vp + h * D;
  const int qt = qblk * 4 + wave;
  const int q = qt * 16 + c_;
  const bool qv = q < g.Lq;
  Vec8<T> qf[DS];
#pragma unroll
  for (int ds = 0; ds < DS; ++ds) qf[ds] = hd_load<T>(qb + hd_row<WX>(g, qrow0, b, qv ? q : 0) * ldq, ds * 32 + g_ * 8, D, qv);
  int nwin = 0;                                                // (WX) the window of this problem: its slice of the mask
  bool add = false;                                            // (WX) a bias or a mask is given (block-uniform)
  if constexpr (WX) { nwin = b % g.nW; add = g.bias != nullptr || g.mask != nullptr; }
  float m_run = -INFINITY, l_run = 0.f;
  f32x4 oacc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < g.Lk; k0 += HD_KB) {
    __syncthreads();                                           // the previous block's Vt readers are done
    hd_stage_t<T, DP, WX>(vt, vb, ld, row0, k0, g.Lk, D, g, b);
    __syncthreads();
    f32x4 st[4];
    float mb = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      st[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int key = k0 + kt * 16 + c_;
      const bool kv = key < g.Lk;
      const T* kp = kb + hd_row<WX>(g, row0, b, kv ? key : 0) * ld;
#pragma unroll
      for (int ds = 0; ds < DS; ++ds) mma16(hd_load<T>(kp, ds * 32 + g_ * 8, D, kv), qf[ds], st[kt]);   // S^T[key][q = c_]
      acc_settle(st[kt]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kk = k0 + kt * 16 + g_ * 4 + r;
        float sv = kk < g.Lk ? st[kt][r] * g.scale : -INFINITY;
        if constexpr (WX) {
          if (add && qv && kk < g.Lk) sv += hdw_add(g, h, nwin, q, kk);         // fp32, before the online softmax; masked: -inf
        }
        st[kt][r] = sv;
        mb = fmaxf(mb, sv);
      }
    }
    mb = fmaxf(mb, shfl_xor_f(mb, 16));
    mb = fmaxf(mb, shfl_xor_f(mb, 32));
    const float m_new = fmaxf(m_run, mb);                      // finite: every block holds at least one real key
    // (WX) a key block that is fully masked for this query while nothing was seen before leaves m_new = -inf (the rule in shifted
    // windows of more than 64 tokens): exponentials are then taken against 0, so that alpha = exp(-inf) = 0 and every p = exp(-inf) = 0
    // and exp(-inf - -inf) never appears.  m_run itself stays -inf until the first unmasked key.
    float m_use = m_new;
    if constexpr (WX) m_use = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __expf(m_run - m_use);                 // exp(-inf) = 0 on the first block
    float lb = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __expf(st[kt][r] - m_use);
        st[kt][r] = p;
        lb += p;
      }
    lb += shfl_xor_f(lb, 16);
    lb += shfl_xor_f(lb, 32);
    l_run = l_run * alpha + lb;
    m_run = m_new;
    // the accumulators hold queries 4 g_ + r (not c_): fetch their rescale factors from the lanes that own them
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a = shfl_f(alpha, 4 * g_ + r);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) oacc[dt][r] *= a;
    }
    if (g.drop.scale != 0.f) {                              // (wave-uniform) F.dropout on the probabilities: scaled keep factors
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) st[kt][r] *= drop_factor(g.drop, (unsigned)bh, q, k0 + kt * 16 + g_ * 4 + r);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      Vec8<T> pf = hd_frag_acc<T>(st[2 * ks], st[2 * ks + 1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) mma16(pf, hd_frag_t<T>(vt + (dt * 16 + c_) * HD_STR + ks * 32, g_), oacc[dt]);
    }
    // the accumulators are next read behind the loop's back edge, the dropout branch or the store predicate: settle them here
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc_settle(oacc[dt]);
  }
  if (qv && g_ == 0) lse[(int64_t)bh * g.Lq + q] = m_run + __logf(l_run);
  const float inv = 1.f / l_run;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float iv = shfl_f(inv, 4 * g_ + r);
    const int qo = qt * 16 + g_ * 4 + r;
    if (qo < g.Lq) {
      T* op = o + hd_row<WX>(g, qrow0, b, qo) * (int64_t)g.hd + h * D + c_;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        if (dt * 16 + c_ < D) op[dt * 16] = from_f32<T>(oacc[dt][r] * iv);
    }
  }
}

// ------------------------------------------------------------------------------------------------- backward: dQ
// grid as the forward; wave <-> query tile; also writes Dq[q] = rowsum(dO o O) for the dK / dV launch
template <typename T, int DP, bool WX = false>
__global__ __launch_bounds__(256) void hdattn_bwd_dq_kernel(const T* __restrict__ qp, const T* __restrict__ kp_, const T* __restrict__ vp,
                                                           const T* __restrict__ oin, const T* __restrict__ dout,
                                                           const float* __restrict__ lse, T* __restrict__ dq,
                                                           float* __restrict__ dsum_out, typename HdG<WX>::type g) {
  constexpr int DS = DP / 32, DT = DP / 16;
  __shared__ __attribute__((aligned(16))) T kt_s[DP * HD_STR];
  const int bh = blockIdx.x / g.qblocks, qblk = blockIdx.x - bh * g.qblocks;
  const int b = bh / g.nH, h = bh - b * g.nH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c_ = lane & 15, g_ = lane >> 4;
  const int D = g.D;
  const int64_t ldq = g.ldq, ld = g.ldkv, qrow0 = (int64_t)b * g.Lq, row0 = (int64_t)b * g.Lk;
  const T* qb = qp + h * D;
  const T* kb = kp_ + h * D;
  const T* vb = vp + h * D;
  const int qt = qblk * 4 + wave;
  const int q = qt * 16 + c_;
  const bool qv = q < g.Lq;
  const int64_t qrow = hd_row<WX>(g, qrow0, b, qv ? q : 0);
  int nwin = 0;
  bool add = false;
  if constexpr (WX) { nwin = b % g.nW; add = g.bias != nullptr || g.mask != nullptr; }
  Vec8<T> qf[DS], dof[DS];
  float dsum = 0.f;
#pragma unroll
  for (int ds = 0; ds < DS; ++ds) {
    const int d0 = ds * 32 + g_ * 8;
    qf[ds] = hd_load<T>(qb + qrow * ldq, d0, D, qv);
    dof[ds] = hd_load<T>(dout + qrow * g.hd + h * D, d0, D, qv);
    Vec8<T> of = hd_load<T>(oin + qrow * g.hd + h * D, d0, D, qv);
#pragma unroll
    for (int e = 0; e < 8; ++e) dsum += of.get(e) * dof[ds].get(e);
  }
  dsum += shfl_xor_f(dsum, 16);
  dsum += shfl_xor_f(dsum, 32);
  const float lq = qv ? lse[(int64_t)bh * g.Lq + q] : INFINITY;          // padded query rows: exp(. - inf) = 0
  if (qv && g_ == 0) dsum_out[(int64_t)bh * g.Lq + q] = dsum;
  f32x4 dqacc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dqacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < g.Lk; k0 += HD_KB) {
    __syncthreads();
    hd_stage_t<T, DP, WX>(kt_s, kb, ld, row0, k0, g.Lk, D, g, b);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      f32x4 dsv[2];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int kt = 2 * ks + half;
        f32x4 pt = f32x4{0.f, 0.f, 0.f, 0.f}, dpt = f32x4{0.f, 0.f, 0.f, 0.f};
        const int key = k0 + kt * 16 + c_;
        const bool kv = key < g.Lk;
        const int64_t krow = hd_row<WX>(g, row0, b, kv ? key : 0);
#pragma unroll
        for (int ds = 0; ds < DS; ++ds) {
          const int d0 = ds * 32 + g_ * 8;
          mma16(hd_load<T>(kb + krow * ld, d0, D, kv), qf[ds], pt);      // S^T [key][q = c_]
          mma16(hd_load<T>(vb + krow * ld, d0, D, kv), dof[ds], dpt);    // dP^T
        }
        acc_settle(pt);                                                 // (read behind hd_drop's branches)
        acc_settle(dpt);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kk = k0 + kt * 16 + g_ * 4 + r;
          float ex = pt[r] * g.scale - lq;                                    // (the product's only use: contracted as in the WX = false kernel)
          if constexpr (WX) {
            if (add && qv && kk < g.Lk) ex += hdw_add(g, h, nwin, q, kk);       // a masked cell: exp(-inf) = 0 exactly, dS = 0
          }
          const float p = kk < g.Lk ? __expf(ex) : 0.f;
          dsv[half][r] = p * (dpt[r] * hd_drop(g, bh, q, kk) - dsum);
        }
      }
      Vec8<T> dsf = hd_frag_acc<T>(dsv[0], dsv[1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) mma16(dsf, hd_frag_t<T>(kt_s + (dt * 16 + c_) * HD_STR + ks * 32, g_), dqacc[dt]);
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc_settle(dqacc[dt]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qo = qt * 16 + g_ * 4 + r;
    if (qo < g.Lq) {
      T* p = dq + hd_row<WX>(g, qrow0, b, qo) * g.lddq + h * D + c_;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        if (dt * 16 + c_ < D) p[dt * 16] = from_f32<T>(dqacc[dt][r] * g.scale);
    }
  }
}

// ------------------------------------------------------------------------------------------------- backward: dK, dV
// grid = B * nH * ceil(Lk / 64); wave <-> key tile; walks the queries in blocks of 64 (Qt, dOt staged transposed)
template <typename T, int DP, bool WX = false>
__global__ __launch_bounds__(256) void hdattn_bwd_dkv_kernel(const T* __restrict__ qp, const T* __restrict__ kp_, const T* __restrict__ vp,
                                                            const T* __restrict__ dout, const float* __restrict__ lse,
                                                            const float* __restrict__ dsum_in, T* __restrict__ dk, T* __restrict__ dv,
                                                            typename HdG<WX>::type g) {
  constexpr int DS = DP / 32, DT = DP / 16;
  __shared__ __attribute__((aligned(16))) T qt_s[DP * HD_STR];
  __shared__ __attribute__((aligned(16))) T dot_s[DP * HD_STR];
  __shared__ float lse_s[HD_KB], dsum_s[HD_KB];
  const int bh = blockIdx.x / g.kblocks, kblk = blockIdx.x - bh * g.kblocks;
  const int b = bh / g.nH, h = bh - b * g.nH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c_ = lane & 15, g_ = lane >> 4;
  const int D = g.D;
  const int64_t ldq = g.ldq, ld = g.ldkv, qrow0 = (int64_t)b * g.Lq, row0 = (int64_t)b * g.Lk;
  const T* qb = qp + h * D;
  const T* kb = kp_ + h * D;
  const T* vb = vp + h * D;
  const T* dob = dout + h * D;
  const int kt = kblk * 4 + wave;
  const int key = kt * 16 + c_;
  const bool kv = key < g.Lk;
  const int64_t krow = hd_row<WX>(g, row0, b, kv ? key : 0);
  int nwin = 0;
  bool add = false;
  if constexpr (WX) { nwin = b % g.nW; add = g.bias != nullptr || g.mask != nullptr; }
  Vec8<T> kf[DS], vf[DS];
#pragma unroll
  for (int ds = 0; ds < DS; ++ds) {
    kf[ds] = hd_load<T>(kb + krow * ld, ds * 32 + g_ * 8, D, kv);
    vf[ds] = hd_load<T>(vb + krow * ld, ds * 32 + g_ * 8, D, kv);
  }
  f32x4 dkacc[DT], dvacc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) { dkacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dvacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  for (int q0 = 0; q0 < g.Lq; q0 += HD_KB) {
    __syncthreads();
    hd_stage_t<T, DP, WX>(qt_s, qb, ldq, qrow0, q0, g.Lq, D, g, b);
    hd_stage_t<T, DP, WX>(dot_s, dob, (int64_t)g.hd, qrow0, q0, g.Lq, D, g, b);
    if (threadIdx.x < HD_KB) {
      const int qq = q0 + threadIdx.x;
      lse_s[threadIdx.x] = qq < g.Lq ? lse[(int64_t)bh * g.Lq + qq] : INFINITY;      // padded queries: p = 0
      dsum_s[threadIdx.x] = qq < g.Lq ? dsum_in[(int64_t)bh * g.Lq + qq] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int qs = 0; qs < 2; ++qs) {
      f32x4 pp[2], dss[2];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int qtl = 2 * qs + half;
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
        const int q = q0 + qtl * 16 + c_;
        const bool qv = q < g.Lq;
        const int64_t qrow = hd_row<WX>(g, qrow0, b, qv ? q : 0);
#pragma unroll
        for (int ds = 0; ds < DS; ++ds) {
          const int d0 = ds * 32 + g_ * 8;
          mma16(hd_load<T>(qb + qrow * ldq, d0, D, qv), kf[ds], s);            // S [q][key = c_]
          mma16(hd_load<T>(dob + qrow * g.hd, d0, D, qv), vf[ds], dp);         // dP
        }
        acc_settle(s);                                                         // (read behind hd_drop's branches)
        acc_settle(dp);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ql = qtl * 16 + g_ * 4 + r;
          float ex = s[r] * g.scale - lse_s[ql];
          if constexpr (WX) {
            if (add && kv && q0 + ql < g.Lq) ex += hdw_add(g, h, nwin, q0 + ql, key);
          }
          const float p = kv ? __expf(ex) : 0.f;
          const float f = hd_drop(g, bh, q0 + ql, key);
          pp[half][r] = p * f;
          dss[half][r] = p * (dp[r] * f - dsum_s[ql]);
        }
      }
      Vec8<T> pf = hd_frag_acc<T>(pp[0], pp[1]);
      Vec8<T> dsf = hd_frag_acc<T>(dss[0], dss[1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        mma16(pf, hd_frag_t<T>(dot_s + (dt * 16 + c_) * HD_STR + qs * 32, g_), dvacc[dt]);
        mma16(dsf, hd_frag_t<T>(qt_s + (dt * 16 + c_) * HD_STR + qs * 32, g_), dkacc[dt]);
      }
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) { acc_settle(dvacc[dt]); acc_settle(dkacc[dt]); }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ko = kt * 16 + g_ * 4 + r;
    if (ko < g.Lk) {
      const int64_t off = hd_row<WX>(g, row0, b, ko) * g.lddkv + h * D + c_;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        if (dt * 16 + c_ < D) {
          dk[off + dt * 16] = from_f32<T>(dkacc[dt][r] * g.scale);
          dv[off + dt * 16] = from_f32<T>(dvacc[dt][r]);
        }
    }
  }
}

// ------------------------------------------------------------------------------------------------- backward: d bias (window / halo entries)
// dbias[h][q][key] = sum over the problems of dS (the arithmetic of lattn_bwd_dbias_kernel, attention_long.hip, plus the mask and the
// window addressing).  One workgroup per (key tile of 16, query block of 64, head) walking ALL problems leaves Swin's stage 1 (8192
// problems of 49 tokens) on a dozen workgroups, so the problems are cut into `nslab` contiguous slabs: grid = (key tiles, query blocks,
// nH * nslab), workgroup (.., .., h * nslab + s) walks the problems [s * per, (s + 1) * per) in order and owns its tile of
// part[s][h][Lq][Lk]; hdw_dbias_reduce_kernel then adds the slabs in slab order.  Fixed order, no atomics.  nslab == 1: part = dbias.
template <typename T, int DP>
__global__ __launch_bounds__(256) void hdattn_bwd_dbias_kernel(const T* __restrict__ qp, const T* __restrict__ kp_, const T* __restrict__ vp,
                                                              const T* __restrict__ dout, const float* __restrict__ lse,
                                                              const float* __restrict__ dsum_in, float* __restrict__ part, int nprob,
                                                              int nslab, HdwGeom g) {
  constexpr int DS = DP / 32;
  const int h = blockIdx.z / nslab, slab = blockIdx.z - h * nslab;
  const int per = (nprob + nslab - 1) / nslab;
  const int p0 = slab * per, p1 = min(nprob, p0 + per);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c_ = lane & 15, g_ = lane >> 4;
  const int D = g.D;
  const int key = blockIdx.x * 16 + c_;
  const bool kv = key < g.Lk;
  const int qt = blockIdx.y * 4 + wave;
  if (qt * 16 >= g.Lq) return;                                   // (no barrier in this kernel)
  const int q = qt * 16 + c_;
  const bool qv = q < g.Lq;
  const int64_t cells = (int64_t)g.Lq * g.Lk;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int p = p0; p < p1; ++p) {
    const int bh = p * g.nH + h, nwin = p % g.nW;
    const int64_t qrow = hd_row<true>(g, (int64_t)p * g.Lq, p, qv ? q : 0), krow = hd_row<true>(g, (int64_t)p * g.Lk, p, kv ? key : 0);
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) {
      const int d0 = ds * 32 + g_ * 8;
      const Vec8<T> kf = hd_load<T>(kp_ + krow * g.ldkv + h * D, d0, D, kv);
      const Vec8<T> vf = hd_load<T>(vp + krow * g.ldkv + h * D, d0, D, kv);
      mma16(hd_load<T>(qp + qrow * g.ldq + h * D, d0, D, qv), kf, s);          // S [q = 16 qt + 4 g + r][key = c]
      mma16(hd_load<T>(dout + qrow * g.hd + h * D, d0, D, qv), vf, dp);        // dP
    }
    acc_settle(s);
    acc_settle(dp);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qq = qt * 16 + g_ * 4 + r;
      if (qq < g.Lq && kv) {
        const float pr = __expf(s[r] * g.scale - lse[(int64_t)bh * g.Lq + qq] + hdw_add(g, h, nwin, qq, key));   // as the dQ kernel
        acc[r] += pr * (dp[r] * hd_drop(g, bh, qq, key) - dsum_in[(int64_t)bh * g.Lq + qq]);
      }
    }
  }
  float* out = part + ((int64_t)slab * g.nH + h) * cells;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qq = qt * 16 + g_ * 4 + r;
    if (qq < g.Lq && kv) out[(int64_t)qq * g.Lk + key] = acc[r];
  }
}
// out[i] = part[0][i] + part[1][i] + ... in slab order (n = nH * Lq * Lk, any n)
__global__ void hdw_dbias_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int64_t n, int nslab) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float s = part[i];
    for (int z = 1; z < nslab; ++z) s += part[(int64_t)z * n + i];
    out[i] = s;
  }
}

// ------------------------------------------------------------------------------------------------- host
template <typename T, int DP>
static int hd_fwd_t(const void* q, const void* k, const void* v, void* o, float* lse, int B, const HdGeom& g, hipStream_t st) {
  hipLaunchKernelGGL((hdattn_fwd_kernel<T, DP>), dim3((unsigned)(B * g.nH * g.qblocks)), dim3(256), 0, st, (const T*)q, (const T*)k,
                     (const T*)v, (T*)o, lse, g);
  return vtx_check_launch();
}
template <typename T, int DP>
static int hd_bwd_t(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, void* dq, void* dk,
                    void* dv, float* ws, int B, const HdGeom& g, hipStream_t st) {
  hipLaunchKernelGGL((hdattn_bwd_dq_kernel<T, DP>), dim3((unsigned)(B * g.nH * g.qblocks)), dim3(256), 0, st, (const T*)q, (const T*)k,
                     (const T*)v, (const T*)o, (const T*)dout, lse, (T*)dq, ws, g);
  int rc = vtx_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL((hdattn_bwd_dkv_kernel<T, DP>), dim3((unsigned)(B * g.nH * g.kblocks)), dim3(256), 0, st, (const T*)q, (const T*)k,
                     (const T*)v, (const T*)dout, lse, (const float*)ws, (T*)dk, (T*)dv, g);
  return vtx_check_launch();
}

#define HD_DISPATCH_T(FN, T, ...)                                                                     \
  (D <= 32 ? FN<T, 32>(__VA_ARGS__) : D <= 64 ? FN<T, 64>(__VA_ARGS__) : D <= 96 ? FN<T, 96>(__VA_ARGS__) : FN<T, 128>(__VA_ARGS__))
#define HD_DISPATCH(FN, ...) (dtype == VTX_BF16 ? HD_DISPATCH_T(FN, bf16, __VA_ARGS__) : HD_DISPATCH_T(FN, float, __VA_ARGS__))

static bool hd_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Everything that is refused, before any launch: the geometry, the strides (every row must hold its nH * D columns; 8-element vectors
// need strides that are multiples of 8 and 16-byte aligned bases) and the dropout arguments (keep_cells = the cells of the mask the
// caller holds, which must be B * nH * Lq * Lk).
static int hd_geom(HdGeom& g, int B, int Lq, int Lk, int nH, int D, int dtype, int64_t ldq, int64_t ldkv, int64_t lddq, int64_t lddkv,
                   float drop_p, uint64_t seed, const uint8_t* keep, int64_t keep_cells) {
  if (dtype != VTX_BF16 && dtype != VTX_F32) return VTX_ERR_DTYPE;
  if (B <= 0 || Lq <= 0 || Lk <= 0 || nH <= 0 || D < 8 || D > 128 || D % 8 != 0) return VTX_ERR_SHAPE;
  if ((int64_t)B * Lq >= 0x7fffffffLL || (int64_t)B * Lk >= 0x7fffffffLL || (int64_t)nH * D >= 0x7fffffffLL) return VTX_ERR_SHAPE;
  const int64_t hd = (int64_t)nH * D;
  if (ldq < hd || ldkv < hd || lddq < hd || lddkv < hd) return VTX_ERR_SHAPE;
  if (ldq % 8 || ldkv % 8 || lddq % 8 || lddkv % 8) return VTX_ERR_ALIGN;
  const int qblocks = (Lq + HD_KB - 1) / HD_KB, kblocks = (Lk + HD_KB - 1) / HD_KB;
  if ((int64_t)B * nH * qblocks >= 0x7fffffffLL || (int64_t)B * nH * kblocks >= 0x7fffffffLL) return VTX_ERR_SHAPE;
  g = HdGeom{Lq, Lk, nH, D, (int)hd, qblocks, kblocks, ldq, ldkv, lddq, lddkv, 1.0f / sqrtf((float)D), DropArgs{}};
  if (drop_p != 0.f) {
    int rc = drop_args(g.drop, drop_p, seed, keep, Lq, Lk);
    if (rc) return rc;
    if ((int64_t)Lq * Lk >= 0x7fffffffLL) return VTX_ERR_SHAPE;          // the hash's cell counter is 32 bits
    if (keep != nullptr && keep_cells != (int64_t)B * nH * Lq * Lk) return VTX_ERR_SHAPE;
  } else if (keep != nullptr) {
    return VTX_ERR_SHAPE;
  }
  return VTX_OK;
}

extern "C" {

int vtx_attn_hd_fwd(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldkv, void* o, float* lse, int B, int Lq, int Lk,
                    int nH, int D, int dtype, float drop_p, uint64_t seed, const uint8_t* keep, int64_t keep_cells, void* stream) {
  if (!q || !k || !v || !o || !lse) return VTX_ERR_NULL;
  HdGeom g;
  int rc = hd_geom(g, B, Lq, Lk, nH, D, dtype, ldq, ldkv, ldq, ldkv, drop_p, seed, keep, keep_cells);
  if (rc) return rc;
  if (!hd_aligned(q) || !hd_aligned(k) || !hd_aligned(v) || !hd_aligned(o)) return VTX_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  return HD_DISPATCH(hd_fwd_t, q, k, v, o, lse, B, g, st);
}

size_t vtx_attn_hd_bwd_workspace(int B, int Lq, int nH) {
  if (B <= 0 || Lq <= 0 || nH <= 0) return 0;
  return (size_t)B * nH * Lq * sizeof(float);                 // Dq = rowsum(dO o O) per (image, head, query)
}

int vtx_attn_hd_bwd(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldkv, const void* o, const void* dout,
                    const float* lse, void* dq, void* dk, void* dv, int64_t lddq, int64_t lddkv, void* workspace, size_t ws_bytes, int B,
                    int Lq, int Lk, int nH, int D, int dtype, float drop_p, uint64_t seed, const uint8_t* keep, int64_t keep_cells,
                    void* stream) {
  if (!q || !k || !v || !o || !dout || !lse || !dq || !dk || !dv || !workspace) return VTX_ERR_NULL;
  HdGeom g;
  int rc = hd_geom(g, B, Lq, Lk, nH, D, dtype, ldq, ldkv, lddq, lddkv, drop_p, seed, keep, keep_cells);
  if (rc) return rc;
  if (ws_bytes < vtx_attn_hd_bwd_workspace(B, Lq, nH)) return VTX_ERR_WORKSPACE;
  if (!hd_aligned(q) || !hd_aligned(k) || !hd_aligned(v) || !hd_aligned(o) || !hd_aligned(dout) || !hd_aligned(dq) || !hd_aligned(dk) ||
      !hd_aligned(dv) || ((uintptr_t)workspace & 3))
    return VTX_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  return HD_DISPATCH(hd_bwd_t, q, k, v, o, dout, lse, dq, dk, dv, (float*)workspace, B, g, st);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------- host: the window / halo entries
template <typename T, int DP>
static int hdw_fwd_t(const void* q, const void* k, const void* v, void* o, float* lse, int nprob, const HdwGeom& g, hipStream_t st) {
  hipLaunchKernelGGL((hdattn_fwd_kernel<T, DP, true>), dim3((unsigned)(nprob * g.nH * g.qblocks)), dim3(256), 0, st, (const T*)q,
                     (const T*)k, (const T*)v, (T*)o, lse, g);
  return vtx_check_launch();
}
template <typename T, int DP>
static int hdw_bwd_t(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, void* dq, void* dk,
                     void* dv, float* dbias, float* ws, float* part, int nslab, int nprob, const HdwGeom& g, hipStream_t st) {
  hipLaunchKernelGGL((hdattn_bwd_dq_kernel<T, DP, true>), dim3((unsigned)(nprob * g.nH * g.qblocks)), dim3(256), 0, st, (const T*)q,
                     (const T*)k, (const T*)v, (const T*)o, (const T*)dout, lse, (T*)dq, ws, g);
  int rc = vtx_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL((hdattn_bwd_dkv_kernel<T, DP, true>), dim3((unsigned)(nprob * g.nH * g.kblocks)), dim3(256), 0, st, (const T*)q,
                     (const T*)k, (const T*)v, (const T*)dout, lse, (const float*)ws, (T*)dk, (T*)dv, g);
  rc = vtx_check_launch();
  if (rc || dbias == nullptr) return rc;
  hipLaunchKernelGGL((hdattn_bwd_dbias_kernel<T, DP>), dim3((unsigned)((g.Lk + 15) / 16), (unsigned)g.qblocks, (unsigned)(g.nH * nslab)),
                     dim3(256), 0, st, (const T*)q, (const T*)k, (const T*)v, (const T*)dout, lse, (const float*)ws,
                     nslab > 1 ? part : dbias, nprob, nslab, g);
  rc = vtx_check_launch();
  if (rc || nslab == 1) return rc;
  const int64_t n = (int64_t)g.nH * g.Lq * g.Lk;
  const int64_t nb = (n + 255) / 256;
  hipLaunchKernelGGL(hdw_dbias_reduce_kernel, dim3((unsigned)(nb > 4096 ? 4096 : nb)), dim3(256), 0, st, (const float*)part, dbias, n,
                     nslab);
  return vtx_check_launch();
}

// slabs of the bias-gradient launch: enough workgroups to fill the device (about 2048), at most 64 slabs, at most one per problem
static int hdw_slabs(int64_t nprob, int Lq, int Lk, int nH) {
  const int64_t tiles = (int64_t)((Lk + 15) / 16) * ((Lq + HD_KB - 1) / HD_KB) * nH;
  int64_t n = 2048 / (tiles < 1 ? 1 : tiles);
  if (n > 64) n = 64;
  if (n > nprob) n = nprob;
  if (n * nH > 65535) n = 65535 / nH;
  if (n < 1) n = 1;
  const int64_t per = (nprob + n - 1) / n;                        // problems per slab; then no more slabs than hold a problem
  return (int)((nprob + per - 1) / per);
}
// problems of a call (0: a geometry that is refused)
static int64_t hdw_problems(int B, int Lq, int Lk, int H, int W, int win) {
  if (B <= 0) return 0;
  if (win == 0) return B;
  if (win < 0 || H <= 0 || W <= 0 || H % win || W % win || (int64_t)win * win != Lq || Lq != Lk) return 0;
  return (int64_t)B * (H / win) * (W / win);
}
static size_t hdw_dsum_floats(int64_t nprob, int Lq, int nH) { return ((size_t)nprob * nH * Lq + 3) & ~(size_t)3; }

static int hdw_geom(HdwGeom& g, int64_t& nprob, const float* bias, const uint8_t* mask, int B, int Lq, int Lk, int nH, int D, int H, int W,
                    int win, int shift, int dtype, int64_t ldq, int64_t ldkv, int64_t lddq, int64_t lddkv, float drop_p, uint64_t seed,
                    const uint8_t* keep, int64_t keep_cells) {
  if (B <= 0 || Lq <= 0 || Lk <= 0) return VTX_ERR_SHAPE;
  nprob = hdw_problems(B, Lq, Lk, H, W, win);
  if (nprob <= 0 || nprob >= 0x7fffffffLL) return VTX_ERR_SHAPE;
  if (mask != nullptr && win == 0) return VTX_ERR_SHAPE;          // the mask is per window
  HdGeom base;
  int rc = hd_geom(base, (int)nprob, Lq, Lk, nH, D, dtype, ldq, ldkv, lddq, lddkv, drop_p, seed, keep, keep_cells);
  if (rc) return rc;
  if ((int64_t)nH * Lq * Lk >= 0x7fffffffLL) return VTX_ERR_SHAPE;
  static_cast<HdGeom&>(g) = base;
  g.bias = bias; g.mask = mask;
  g.H = H; g.W = W; g.win = win; g.shift = (win && shift) ? win / 2 : 0;
  g.nWx = win ? W / win : 1; g.nW = win ? (H / win) * (W / win) : 1;
  return VTX_OK;
}

#define HDW_DISPATCH_T(FN, T, ...)                                                                    \
  (D <= 32 ? FN<T, 32>(__VA_ARGS__) : D <= 64 ? FN<T, 64>(__VA_ARGS__) : D <= 96 ? FN<T, 96>(__VA_ARGS__) : FN<T, 128>(__VA_ARGS__))
#define HDW_DISPATCH(FN, ...) (dtype == VTX_BF16 ? HDW_DISPATCH_T(FN, bf16, __VA_ARGS__) : HDW_DISPATCH_T(FN, float, __VA_ARGS__))

extern "C" {

int vtx_attn_hdw_fwd(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldkv, void* o, float* lse, const float* bias,
                     const uint8_t* mask, int B, int Lq, int Lk, int nH, int D, int H, int W, int win, int shift, int dtype, float drop_p,
                     uint64_t seed, const uint8_t* keep, int64_t keep_cells, void* stream) {
  if (!q || !k || !v || !o || !lse) return VTX_ERR_NULL;
  HdwGeom g;
  int64_t nprob;
  int rc = hdw_geom(g, nprob, bias, mask, B, Lq, Lk, nH, D, H, W, win, shift, dtype, ldq, ldkv, ldq, ldkv, drop_p, seed, keep, keep_cells);
  if (rc) return rc;
  if (!hd_aligned(q) || !hd_aligned(k) || !hd_aligned(v) || !hd_aligned(o) || ((uintptr_t)bias & 3)) return VTX_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  return HDW_DISPATCH(hdw_fwd_t, q, k, v, o, lse, (int)nprob, g, st);
}

size_t vtx_attn_hdw_bwd_workspace(int B, int Lq, int Lk, int nH, int H, int W, int win, int has_bias) {
  if (Lq <= 0 || Lk <= 0 || nH <= 0) return 0;
  const int64_t nprob = hdw_problems(B, Lq, Lk, H, W, win);
  if (nprob <= 0) return 0;
  size_t fl = hdw_dsum_floats(nprob, Lq, nH);                     // Dq = rowsum(dO o O) per (problem, head, query)
  if (has_bias) {
    const int nslab = hdw_slabs(nprob, Lq, Lk, nH);
    if (nslab > 1) fl += (size_t)nslab * nH * Lq * Lk;            // part[slab][nH][Lq][Lk]
  }
  return fl * sizeof(float);
}

int vtx_attn_hdw_bwd(const void* q, const void* k, const void* v, int64_t ldq, int64_t ldkv, const void* o, const void* dout,
                     const float* lse, const float* bias, const uint8_t* mask, void* dq, void* dk, void* dv, int64_t lddq, int64_t lddkv,
                     float* dbias, void* workspace, size_t ws_bytes, int B, int Lq, int Lk, int nH, int D, int H, int W, int win, int shift,
                     int dtype, float drop_p, uint64_t seed, const uint8_t* keep, int64_t keep_cells, void* stream) {
  if (!q || !k || !v || !o || !dout || !lse || !dq || !dk || !dv || !workspace) return VTX_ERR_NULL;
  if ((bias == nullptr) != (dbias == nullptr)) return VTX_ERR_SHAPE;
  HdwGeom g;
  int64_t nprob;
  int rc = hdw_geom(g, nprob, bias, mask, B, Lq, Lk, nH, D, H, W, win, shift, dtype, ldq, ldkv, lddq, lddkv, drop_p, seed, keep,
                    keep_cells);
  if (rc) return rc;
  if (ws_bytes < vtx_attn_hdw_bwd_workspace(B, Lq, Lk, nH, H, W, win, bias != nullptr)) return VTX_ERR_WORKSPACE;
  if (!hd_aligned(q) || !hd_aligned(k) || !hd_aligned(v) || !hd_aligned(o) || !hd_aligned(dout) || !hd_aligned(dq) || !hd_aligned(dk) ||
      !hd_aligned(dv) || ((uintptr_t)workspace & 3) || ((uintptr_t)bias & 3) || ((uintptr_t)dbias & 3))
    return VTX_ERR_ALIGN;
  const int nslab = bias ? hdw_slabs(nprob, Lq, Lk, nH) : 1;
  float* ws = (float*)workspace;
  float* part = ws + hdw_dsum_floats(nprob, Lq, nH);
  hipStream_t st = (hipStream_t)stream;
  return HDW_DISPATCH(hdw_bwd_t, q, k, v, o, dout, lse, dq, dk, dv, dbias, ws, part, nslab, (int)nprob, g, st);
}

}  // extern "C"
