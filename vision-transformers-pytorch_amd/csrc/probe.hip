// Linear-probe evaluation of frozen features (the second protocol DINO runs are judged by) on the device: H linear heads,
// one per (learning rate, weight decay) pair, trained at once on the rows of a feature bank.  The (rows, classes) logit
// matrix is never written: the forward keeps a running softmax per row, the backward recomputes the logits tile.
//
//   probe_fwd_kernel    one 256-thread workgroup per (head, tile of 64 rows).  Wave w owns rows 16 w .. 16 w + 15 of the tile:
//                       their MFMA A-operand fragments stay resident (registers while D allows it, otherwise re-read through
//                       L1 / L2).  The head's class rows stream through ONE LDS tile of TN = 64 / 32 / 16 rows in ascending
//                       class order, as knn_search_kernel streams the bank: every thread loads its 16-byte pieces of tile t + 1
//                       into registers before the products of tile t.  A logit is the fp32-accumulated dot product of its two
//                       rows -- v_mfma_f32_16x16x32_bf16 (bf16) or 8 x v_mfma_f32_16x16x4_f32 (fp32, exact) per 32 columns of
//                       D, the SAME chain for every pair -- plus one fp32 add of the bias.  The lane that sees a row's logits
//                       of classes col, col + 16, ... keeps their running maximum, the rescaled running sum of
//                       __expf(x - max), the first class of the highest logit and the label's logit; the 16 lanes of a row
//                       meet once, in a fixed butterfly, at the end.  Pad classes of the last tile are masked: they add nothing
//                       to the sum and are never a candidate.
//   probe_meter_kernel  one workgroup adds the batch to the fp64 meter [H, 3] in a fixed order (as knn_meter_kernel).
//   probe_bwd_kernel    one workgroup per (row slab, head, chunk of D, tile of 64 classes); wave w owns 16 classes.  Per step
//                       of 32 rows: the workgroup stages the rows' chunk TRANSPOSED in LDS; every wave recomputes its
//                       32 x 16 logits with the forward's chain, forms g = (__expf(x - lse) - [c == label]) * scale in fp32,
//                       and hands g from the accumulator registers to the A operand of a second MFMA as they lie (lane
//                       (class, group) holds 8 rows of its class: the 8 k-slots), rounded to bf16 in bf16 mode.  The B
//                       operand -- the same 8 rows of 16 columns of D -- is two 8-byte (16-byte in fp32) LDS reads of the
//                       transposed tile.  dW accumulates in registers (NDT 16-column tiles: D chunks of 128 / 384 / 512
//                       columns; D > 512 runs two chunks that each recompute the logits), db in fp32 from the unrounded g.
//   probe_reduce_kernel slabs > 1: out[i] = sum over slabs, in slab order.
//   probe_sgd_kernel    one launch over all heads: torch.optim.SGD with momentum on fp32 masters, the bf16 shadow written in
//                       the same pass.  Contraction is off: every product and sum is rounded on its own.
//
// No floating-point atomics anywhere; every sum has a fixed order, so the same inputs give the same bits.
#include "vtx_common.h"

#define PROBE_TN_MAX 64      // class rows of an LDS tile at most
#define PROBE_STAGE 16       // 16-byte pieces of a class tile a thread holds in flight (16 * 256 * 16 B = 64 KiB)
#define PROBE_MAX_D 1024
#define PROBE_MAX_H 32
#define PROBE_TM 64          // rows of a forward workgroup
#define PROBE_TC 64          // classes of a backward workgroup
#define PROBE_STEP 32        // rows of a backward step: the 8 k-slots of 4 lane groups
#define PROBE_MAX_SLABS 64
#define PROBE_SLAB_ROWS 128  // no slab below this many rows

struct ProbeRates { float lr[PROBE_MAX_H]; float wd[PROBE_MAX_H]; };      // by value: 256 B of kernel argument

__device__ __forceinline__ float probe_low() { return -3.0e38f; }         // a finite "no logit yet": exp(low - x) = 0, low - low = 0

// row of x that row m of the call reads: rows[m] or m, never outside [0, N)
__device__ __forceinline__ int64_t probe_row(const int32_t* __restrict__ rows, int m, int N) {
  int r = rows ? rows[m] : m;
  r = r < 0 ? 0 : (r > N - 1 ? N - 1 : r);
  return (int64_t)r;
}

// ------------------------------------------------------------------------------------------------ forward
// NCH > 0: the row fragments of NCH 32-column chunks of D live in registers (chunks past D are zero and add nothing);
// NCH == 0: any D, the fragments are re-read from global memory for every class tile.
template <typename T, int NCH>
__global__ __launch_bounds__(256) void probe_fwd_kernel(const T* __restrict__ x, const int32_t* __restrict__ rows,
                                                       const int64_t* __restrict__ labels, const T* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ lse,
                                                       float* __restrict__ ce, int32_t* __restrict__ pred, int M, int N,
                                                       int C, int D, int nrt, int TN) {
  extern __shared__ __attribute__((aligned(16))) unsigned char probe_smem[];
  constexpr int ES = (int)sizeof(T);
  unsigned char* bt = probe_smem;                                       // [TN][pitch] the class tile
  const int pitch = D * ES + 16;                                        // +16 B: rows 16 B apart in the 256-B bank row

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int rt = (int)(blockIdx.x % (unsigned)nrt), h = (int)(blockIdx.x / (unsigned)nrt);
  const int m0 = rt * PROBE_TM + wave * 16;                             // first row of this wave
  const T* wh = w + (int64_t)h * C * D;
  const float* bh = bias ? bias + (int64_t)h * C : nullptr;
  const int ntiles = (C + TN - 1) / TN;
  const int nch = (D + 31) >> 5;
  const int nblk = TN >> 4;

  // the row of this lane's A fragment (rows past M repeat row M - 1; nothing of them is written out)
  int ra = m0 + col;
  if (ra > M - 1) ra = M - 1;
  const T* qrow = x + probe_row(rows, ra, N) * D;
  Vec8<T> qf[NCH > 0 ? NCH : 1];
  if constexpr (NCH > 0) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int kk = c * 32 + g * 8;
      qf[c] = load8_clamped<T>(qrow + (kk < D ? kk : 0), kk < D);
    }
  }
  // the rows whose logits this lane sees: m0 + 4 g + r; their labels as a class in [0, C), or -1: never used as an index
  int32_t lab[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int m = m0 + 4 * g + r;
    if (m > M - 1) m = M - 1;
    const int64_t lb = labels[probe_row(rows, m, N)];
    lab[r] = (lb >= 0 && lb < (int64_t)C) ? (int32_t)lb : -1;
  }
  float mx[4], sm[4], bv[4], xl[4];
  int32_t bc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { mx[r] = probe_low(); sm[r] = 0.f; bv[r] = -INFINITY; bc[r] = 0x7fffffff; xl[r] = -INFINITY; }

  // this thread's 16-byte pieces of a class tile: piece v = tid + 256 i is bytes [16 pc, 16 pc + 16) of tile row pr
  const int vpr = (D * ES) >> 4;
  const int nvec = TN * vpr;
  const int pr0 = tid / vpr, pc0 = tid - pr0 * vpr, dpr = 256 / vpr, dpc = 256 - dpr * vpr;
  uint4 st[PROBE_STAGE];

  // tt = -1 only brings tile 0 in
  for (int tt = -1; tt < ntiles; ++tt) {
    const int row0 = tt * TN;
    const bool more = tt + 1 < ntiles;
    if (more) {
      int pr = pr0, pc = pc0;
#pragma unroll
      for (int i = 0; i < PROBE_STAGE; ++i) {
        int gr = row0 + TN + pr;
        if (gr > C - 1) gr = C - 1;                    // pad classes repeat the last class row; their logits are masked
        const uint4* src = reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(wh) + (int64_t)gr * (D * ES) + pc * 16);
        st[i] = tid + 256 * i < nvec ? *src : uint4{0u, 0u, 0u, 0u};
        pr += dpr; pc += dpc;
        if (pc >= vpr) { pc -= vpr; pr += 1; }
      }
    }

    if (tt >= 0) {
      for (int blk = 0; blk < nblk; ++blk) {
        if (row0 + blk * 16 >= C) break;               // (wave-uniform: a block of pad classes only)
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        const unsigned char* brow = bt + (blk * 16 + col) * pitch;
        if constexpr (NCH > 0) {
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            const int kk = c * 32 + g * 8;
            const Vec8<T> bf = load8_clamped<T>(reinterpret_cast<const T*>(brow) + (kk < D ? kk : 0), kk < D);
            mma16(qf[c], bf, acc);
          }
          acc_settle(acc);
        } else {
          for (int c = 0; c < nch; ++c) {
            const int kk = c * 32 + g * 8;
            const int ko = kk < D ? kk : 0;
            const Vec8<T> bf = load8_clamped<T>(reinterpret_cast<const T*>(brow) + ko, kk < D);
            const Vec8<T> a = load8_clamped<T>(qrow + ko, kk < D);
            mma16(a, bf, acc);
            acc_settle(acc);                           // read in the block of the products (vtx_common.h)
          }
        }
        const int j = row0 + blk * 16 + col;           // the class of this lane's logits
        const bool real = j < C;
        const float bj = bh ? bh[real ? j : C - 1] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float s = acc[r] + bj;
          if (real) {
            const float mn = fmaxf(mx[r], s);          // (a NaN logit leaves the maximum and turns the sum into NaN)
            sm[r] = sm[r] * __expf(mx[r] - mn) + __expf(s - mn);
            mx[r] = mn;
            if (s > bv[r]) { bv[r] = s; bc[r] = j; }   // classes ascend: the first of equal logits stays
            if (j == lab[r]) xl[r] = s;
          }
        }
      }
    }
    __syncthreads();                                   // every wave is done with the tile
    if (more) {
      int pr = pr0, pc = pc0;
#pragma unroll
      for (int i = 0; i < PROBE_STAGE; ++i) {
        if (tid + 256 * i < nvec) *reinterpret_cast<uint4*>(bt + pr * pitch + pc * 16) = st[i];
        pr += dpr; pc += dpc;
        if (pc >= vpr) { pc -= vpr; pr += 1; }
      }
    }
    __syncthreads();                                   // the next tile is in place
  }

  // ---- the 16 lanes of a row meet: a fixed butterfly over the lane's low four bits
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int o = 1; o <= 8; o <<= 1) {
      const float om = shfl_xor_f(mx[r], o), os = shfl_xor_f(sm[r], o), ov = shfl_xor_f(bv[r], o), ox = shfl_xor_f(xl[r], o);
      const int32_t oc = __shfl_xor(bc[r], o, 64);
      const float mn = fmaxf(mx[r], om);
      // both sides form the same two products and add them in the same order (lower lane's part first)
      const bool low = (lane & o) == 0;
      const float pa = (low ? sm[r] : os) * __expf((low ? mx[r] : om) - mn);
      const float pb = (low ? os : sm[r]) * __expf((low ? om : mx[r]) - mn);
      sm[r] = pa + pb;
      mx[r] = mn;
      if (ov > bv[r] || (ov == bv[r] && oc < bc[r])) { bv[r] = ov; bc[r] = oc; }
      xl[r] = fmaxf(xl[r], ox);
    }
    const int m = m0 + 4 * g + r;
    if (col == 0 && m < M) {
      const float l = mx[r] + __logf(sm[r]);
      const int64_t o = (int64_t)h * M + m;
      lse[o] = l;
      ce[o] = lab[r] >= 0 ? l - xl[r] : __builtin_nanf("");
      pred[o] = (bc[r] >= 0 && bc[r] < C) ? bc[r] : 0;
    }
  }
}

// meter[h] = [n, loss_sum, top1] += [M, sum of ce over the rows whose label is a class, rows with pred == label].  Thread t
// sums rows t, t + 256, ... in fp64, then a fixed tree over the 256 partials.
__global__ __launch_bounds__(256) void probe_meter_kernel(const float* __restrict__ ce, const int32_t* __restrict__ pred,
                                                         const int64_t* __restrict__ labels, const int32_t* __restrict__ rows,
                                                         double* __restrict__ meter, int M, int N, int C, int H) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x;
  for (int h = 0; h < H; ++h) {
    double ls = 0.0, hit = 0.0;
    for (int m = tid; m < M; m += 256) {
      const int64_t lb = labels[probe_row(rows, m, N)];
      if (lb >= 0 && lb < (int64_t)C) {
        ls += (double)ce[(int64_t)h * M + m];
        if ((int64_t)pred[(int64_t)h * M + m] == lb) hit += 1.0;
      }
    }
    red[0][tid] = ls; red[1][tid] = hit;
    __syncthreads();
    for (int sft = 128; sft >= 1; sft >>= 1) {
      if (tid < sft) { red[0][tid] += red[0][tid + sft]; red[1][tid] += red[1][tid + sft]; }
      __syncthreads();
    }
    if (tid == 0) { meter[3 * h] += (double)M; meter[3 * h + 1] += red[0][0]; meter[3 * h + 2] += red[1][0]; }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ backward
template <typename T> struct ProbeXT;                  // row pitch (elements) of the transposed tile: 32 rows + pad
template <> struct ProbeXT<bf16> { static constexpr int XP = 40; };      // 80 B: 8-byte reads stay aligned
template <> struct ProbeXT<float> { static constexpr int XP = 36; };     // 144 B: 16-byte reads stay aligned

template <typename T, int NDT>
__global__ __launch_bounds__(256) void probe_bwd_kernel(const T* __restrict__ x, const int32_t* __restrict__ rows,
                                                       const int64_t* __restrict__ labels, const T* __restrict__ w,
                                                       const float* __restrict__ bias, const float* __restrict__ lse,
                                                       float* __restrict__ out_w, float* __restrict__ out_b, int M, int N,
                                                       int H, int C, int D, int nct, int nchunk, int per, float scale,
                                                       int64_t slab_stride) {
  extern __shared__ __attribute__((aligned(16))) unsigned char probe_smem[];
  constexpr int XP = ProbeXT<T>::XP;
  T* xt = reinterpret_cast<T*>(probe_smem);                             // [NDT * 16][XP]: column d of the chunk, rows of the step

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  unsigned bid = blockIdx.x;
  const int ct = (int)(bid % (unsigned)nct); bid /= (unsigned)nct;
  const int ch = (int)(bid % (unsigned)nchunk); bid /= (unsigned)nchunk;
  const int h = (int)(bid % (unsigned)H);
  const int sl = (int)(bid / (unsigned)H);
  const int d0 = ch * NDT * 16;
  const int dcols = D - d0 < NDT * 16 ? D - d0 : NDT * 16;              // a multiple of 8
  const int m_beg = sl * per;
  const int m_end = m_beg + per < M ? m_beg + per : M;
  const int nch = (D + 31) >> 5;

  const int cls = ct * PROBE_TC + wave * 16 + col;                      // the class of this lane: B row of the logits, A row of dW
  const bool creal = cls < C;
  const T* wrow = w + ((int64_t)h * C + (creal ? cls : C - 1)) * D;
  const float bj = bias ? bias[(int64_t)h * C + (creal ? cls : C - 1)] : 0.f;
  const float* lh = lse + (int64_t)h * M;

  f32x4 dacc[NDT];
#pragma unroll
  for (int t = 0; t < NDT; ++t) dacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbacc = 0.f;

  const int vpr = dcols >> 3;                                           // 8-element pieces of a row's chunk
  const int nvec = PROBE_STEP * vpr;

  for (int mb = m_beg; mb < m_end; mb += PROBE_STEP) {
    __syncthreads();                                   // every wave is done with the previous step's tile
    for (int v = tid; v < nvec; v += 256) {
      const int pr = v / vpr, pc = v - pr * vpr;
      const int m = mb + pr;
      const bool ok = m < m_end;
      const Vec8<T> p = load8_clamped<T>(x + probe_row(rows, ok ? m : m_end - 1, N) * D + d0 + pc * 8, ok);
#pragma unroll
      for (int e = 0; e < 8; ++e) xt[(pc * 8 + e) * XP + pr] = p.v[e];
    }
    __syncthreads();                                   // the tile is in place

    // ---- logits of rows mb .. mb + 31 x this wave's 16 classes: the forward's chain
    Vec8<T> ga;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      int ma = mb + b * 16 + col;
      if (ma > m_end - 1) ma = m_end - 1;
      const T* xrow = x + probe_row(rows, ma, N) * D;
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int c = 0; c < nch; ++c) {
        const int kk = c * 32 + g * 8;
        const int ko = kk < D ? kk : 0;
        const Vec8<T> a = load8_clamped<T>(xrow + ko, kk < D);
        const Vec8<T> bf = load8_clamped<T>(wrow + ko, kk < D);
        mma16(a, bf, acc);
        acc_settle(acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mb + b * 16 + 4 * g + r;
        const bool ok = m < m_end && creal;
        const int mc = m < m_end ? m : m_end - 1;
        const int64_t lb = labels[probe_row(rows, mc, N)];
        const float s = acc[r] + bj;
        float gv = (__expf(s - lh[mc]) - ((int64_t)cls == lb ? 1.f : 0.f)) * scale;
        gv = ok ? gv : 0.f;
        dbacc += gv;                                   // the unrounded value
        ga.set(b * 4 + r, gv);                         // k-slot b 4 + r of this lane group = row b 16 + 4 g + r of the step
      }
    }
    // ---- dW tile += g^T x: the 8 rows of this lane's k-slots are two runs of 4 in the transposed tile
#pragma unroll
    for (int t = 0; t < NDT; ++t) {
      if (t * 16 < dcols) {                            // (block-uniform)
        const T* xr = xt + (t * 16 + col) * XP + 4 * g;
        Vec8<T> xb;
        if constexpr (sizeof(T) == 2) {
          const bf16x4 lo = *reinterpret_cast<const bf16x4*>(xr), hi = *reinterpret_cast<const bf16x4*>(xr + 16);
#pragma unroll
          for (int e = 0; e < 4; ++e) { xb.v[e] = lo[e]; xb.v[4 + e] = hi[e]; }
        } else {
          const f32x4 lo = *reinterpret_cast<const f32x4*>(xr), hi = *reinterpret_cast<const f32x4*>(xr + 16);
#pragma unroll
          for (int e = 0; e < 4; ++e) { xb.v[e] = lo[e]; xb.v[4 + e] = hi[e]; }
        }
        mma16(ga, xb, dacc[t]);
      }
    }
    // The accumulators are read behind the loop's exit branch, where the compiler does not pad the read with the wait
    // states the matrix pipe needs (profiles/round5_mfma_branch_hazard.md): 16 wait states here cover the last product of
    // every path (an 8-pass MFMA needs 11), once per 32 rows.
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15");
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- dW[class 4 g + r of the wave][d0 + 16 t + col], db[class col] summed over the 4 lane groups in a fixed order
  float* o = out_w + (int64_t)sl * slab_stride;
#pragma unroll
  for (int t = 0; t < NDT; ++t) {
    acc_settle(dacc[t]);
    const int dc = t * 16 + col;
    if (dc < dcols) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = ct * PROBE_TC + wave * 16 + 4 * g + r;
        if (c < C) o[((int64_t)h * C + c) * D + d0 + dc] = dacc[t][r];
      }
    }
  }
  if (ch == 0) {
    float s = dbacc;
    s += shfl_xor_f(s, 16);
    s += shfl_xor_f(s, 32);
    if (g == 0 && creal) out_b[(int64_t)sl * slab_stride + (int64_t)h * C + cls] = s;
  }
}

// dw | db [n] = sum over the slabs of the workspace, in slab order
__global__ __launch_bounds__(256) void probe_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                          float* __restrict__ db, int64_t nw, int64_t n, int slabs) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float s = ws[i];
    for (int z = 1; z < slabs; ++z) s += ws[(int64_t)z * n + i];
    if (i < nw) dw[i] = s; else db[i - nw] = s;
  }
}

// ------------------------------------------------------------------------------------------------ SGD
// torch.optim.SGD (dampening 0, no Nesterov): d = g + wd w; buf = mu buf + d; w = w - lr buf -- each product and each sum
// rounded on its own.  blockIdx.y = head; the head's C D weights, then its C biases.
// A product as its own rounded value.  The library is built with -ffp-contract=fast, under which the backend fuses a
// product into the sum that uses it whatever the pragma below says; it does not fuse across this empty statement.
__device__ __forceinline__ float probe_rounded(float v) { asm volatile("" : "+v"(v)); return v; }

__global__ __launch_bounds__(256) void probe_sgd_kernel(float* __restrict__ w, float* __restrict__ b, float* __restrict__ mw,
                                                       float* __restrict__ mb, const float* __restrict__ dw,
                                                       const float* __restrict__ db, bf16* __restrict__ shadow,
                                                       ProbeRates rates, float mu, int C, int D) {
#pragma clang fp contract(off)
  const int h = blockIdx.y;
  float lr = rates.lr[0], wd = rates.wd[0];
#pragma unroll
  for (int i = 1; i < PROBE_MAX_H; ++i) if (i == h) { lr = rates.lr[i]; wd = rates.wd[i]; }      // (static indices: no scratch copy)
  const int64_t nw = (int64_t)C * D, n = nw + C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const bool isw = i < nw;
    const int64_t e = isw ? (int64_t)h * nw + i : (int64_t)h * C + (i - nw);
    float* pw = isw ? w + e : b + e;
    float* pm = isw ? mw + e : mb + e;
    const float gr = isw ? dw[e] : db[e];
    const float wv = *pw;
    const float t1 = probe_rounded(wd * wv);
    const float d = gr + t1;
    const float t2 = probe_rounded(mu * *pm);
    const float bufv = t2 + d;
    const float t3 = probe_rounded(lr * bufv);
    const float nv = wv - t3;
    *pm = bufv;
    *pw = nv;
    if (isw && shadow) shadow[e] = (bf16)nv;           // round to nearest even
  }
}

// ------------------------------------------------------------------------------------------------ host side
static int probe_shape_check(int64_t M, int64_t N, int H, int C, int D) {
  if (M < 1 || N < 1 || M > N || N >= (1ll << 31) || H < 1 || H > PROBE_MAX_H || C < 1 || D < 1 || D > PROBE_MAX_D)
    return VTX_ERR_SHAPE;
  if ((int64_t)H * C * D >= (1ll << 31)) return VTX_ERR_SHAPE;
  if (D % 8 != 0) return VTX_ERR_ALIGN;
  return VTX_OK;
}

static int probe_ndt(int D) { return D <= 128 ? 8 : (D <= 384 ? 24 : 32); }

// Row slabs of the backward: a function of (M, H, C, D) alone.  As many as fill the 256 CUs with the (head, D chunk, class
// tile) workgroups there are, no slab below 128 rows, 64 at most; a slab is a multiple of the 32-row step.
static void probe_slabs(int64_t M, int H, int C, int D, int* slabs, int* per) {
  const int ndt = probe_ndt(D);
  const int64_t tiles = (int64_t)H * ((C + PROBE_TC - 1) / PROBE_TC) * ((D + ndt * 16 - 1) / (ndt * 16));
  int64_t s = 256 / tiles;
  const int64_t cap = (M + PROBE_SLAB_ROWS - 1) / PROBE_SLAB_ROWS;
  if (s > cap) s = cap;
  if (s > PROBE_MAX_SLABS) s = PROBE_MAX_SLABS;
  if (s < 1) s = 1;
  int64_t p = (M + s - 1) / s;
  p = (p + PROBE_STEP - 1) / PROBE_STEP * PROBE_STEP;
  s = (M + p - 1) / p;                                 // (no empty slab)
  *slabs = (int)s; *per = (int)p;
}

template <typename T, int NCH>
static int probe_fwd_launch(const void* x, const int32_t* rows, const int64_t* labels, const void* w, const float* bias,
                            float* lse, float* ce, int32_t* pred, int M, int N, int H, int C, int D, hipStream_t st) {
  constexpr int ES = (int)sizeof(T);
  int TN = PROBE_TN_MAX;
  while (TN > 16 && TN * D * ES > 65536) TN >>= 1;     // D <= 1024: 16 rows of fp32 are 64 KiB
  const size_t smem = (size_t)TN * (D * ES + 16);
  auto kern = probe_fwd_kernel<T, NCH>;
  if (smem > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
    return VTX_ERR_LAUNCH;
  const int nrt = (M + PROBE_TM - 1) / PROBE_TM;
  if ((int64_t)nrt * H >= (1ll << 31)) return VTX_ERR_SHAPE;
  hipLaunchKernelGGL(kern, dim3((unsigned)(nrt * H)), dim3(256), smem, st, (const T*)x, rows, labels, (const T*)w, bias, lse,
                     ce, pred, M, N, C, D, nrt, TN);
  return VTX_OK;
}

template <typename T, int NDT>
static int probe_bwd_launch(const void* x, const int32_t* rows, const int64_t* labels, const void* w, const float* bias,
                            const float* lse, float* out_w, float* out_b, int M, int N, int H, int C, int D, int slabs, int per,
                            float scale, int64_t slab_stride, hipStream_t st) {
  const size_t smem = (size_t)NDT * 16 * ProbeXT<T>::XP * sizeof(T);
  auto kern = probe_bwd_kernel<T, NDT>;
  if (smem > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
    return VTX_ERR_LAUNCH;
  const int nct = (C + PROBE_TC - 1) / PROBE_TC, nchunk = (D + NDT * 16 - 1) / (NDT * 16);
  const int64_t grid = (int64_t)nct * nchunk * H * slabs;
  if (grid >= (1ll << 31)) return VTX_ERR_SHAPE;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), smem, st, (const T*)x, rows, labels, (const T*)w, bias, lse, out_w,
                     out_b, M, N, H, C, D, nct, nchunk, per, scale, slab_stride);
  return VTX_OK;
}

extern "C" {

/* include/vtx.h: vtx_probe_workspace_bytes */
size_t vtx_probe_workspace_bytes(int64_t M, int H, int C, int D) {
  if (probe_shape_check(M, M, H, C, D) != VTX_OK) return 0;
  int slabs, per;
  probe_slabs(M, H, C, D, &slabs, &per);
  return slabs > 1 ? (size_t)slabs * ((size_t)H * C * D + (size_t)H * C) * 4u : 0;
}

/* include/vtx.h: vtx_probe_fwd */
int vtx_probe_fwd(const void* x, const int32_t* rows, const int64_t* labels, const void* w, const float* bias, float* lse,
                  float* ce, int32_t* pred, double* meter, int64_t M, int64_t N, int H, int C, int D, int dtype,
                  void* stream) {
  if (!x || !labels || !w || !lse || !ce || !pred) return VTX_ERR_NULL;
  const int rc = probe_shape_check(M, N, H, C, D);
  if (rc != VTX_OK) return rc;
  if (dtype != VTX_BF16 && dtype != VTX_F32) return VTX_ERR_DTYPE;
  if (((uintptr_t)x | (uintptr_t)w) & 15u) return VTX_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const int nch = (D + 31) / 32;
  int lr;
#define PROBE_GO(T, NCH) lr = probe_fwd_launch<T, NCH>(x, rows, labels, w, bias, lse, ce, pred, (int)M, (int)N, H, C, D, st)
  if (dtype == VTX_BF16) { if (nch <= 4) PROBE_GO(bf16, 4); else if (nch <= 12) PROBE_GO(bf16, 12); else PROBE_GO(bf16, 0); }
  else { if (nch <= 4) PROBE_GO(float, 4); else PROBE_GO(float, 0); }
#undef PROBE_GO
  if (lr != VTX_OK) return lr;
  if (meter)
    hipLaunchKernelGGL(probe_meter_kernel, dim3(1), dim3(256), 0, st, (const float*)ce, (const int32_t*)pred, labels, rows,
                       meter, (int)M, (int)N, C, H);
  return vtx_check_launch();
}

/* include/vtx.h: vtx_probe_bwd */
int vtx_probe_bwd(const void* x, const int32_t* rows, const int64_t* labels, const void* w, const float* bias,
                  const float* lse, float* dw, float* db, int64_t M, int64_t N, int H, int C, int D, float scale, void* ws,
                  size_t ws_bytes, int dtype, void* stream) {
  if (!x || !labels || !w || !lse || !dw || !db) return VTX_ERR_NULL;
  const int rc = probe_shape_check(M, N, H, C, D);
  if (rc != VTX_OK) return rc;
  if (!(scale > 0.f) || !(scale < INFINITY)) return VTX_ERR_SHAPE;
  if (dtype != VTX_BF16 && dtype != VTX_F32) return VTX_ERR_DTYPE;
  if (((uintptr_t)x | (uintptr_t)w) & 15u) return VTX_ERR_ALIGN;
  int slabs, per;
  probe_slabs(M, H, C, D, &slabs, &per);
  const int64_t nw = (int64_t)H * C * D, n = nw + (int64_t)H * C;
  if (slabs > 1) {
    if (ws_bytes < (size_t)slabs * (size_t)n * 4u) return VTX_ERR_WORKSPACE;
    if (!ws) return VTX_ERR_NULL;
    if ((uintptr_t)ws & 3u) return VTX_ERR_ALIGN;
  }
  hipStream_t st = (hipStream_t)stream;
  float* out_w = slabs > 1 ? (float*)ws : dw;          // partials: [slab][H C D | H C]; one slab writes the outputs themselves
  float* out_b = slabs > 1 ? (float*)ws + nw : db;
  const int ndt = probe_ndt(D);
  int lr;
#define PROBE_GO(T, NDT) lr = probe_bwd_launch<T, NDT>(x, rows, labels, w, bias, lse, out_w, out_b, (int)M, (int)N, H, C, D, slabs, per, scale, slabs > 1 ? n : 0, st)
  if (dtype == VTX_BF16) { if (ndt == 8) PROBE_GO(bf16, 8); else if (ndt == 24) PROBE_GO(bf16, 24); else PROBE_GO(bf16, 32); }
  else { if (ndt == 8) PROBE_GO(float, 8); else if (ndt == 24) PROBE_GO(float, 24); else PROBE_GO(float, 32); }
#undef PROBE_GO
  if (lr != VTX_OK) return lr;
  if (slabs > 1) {
    int64_t nb = (n + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(probe_reduce_kernel, dim3((unsigned)nb), dim3(256), 0, st, (const float*)ws, dw, db, nw, n, slabs);
  }
  return vtx_check_launch();
}

/* include/vtx.h: vtx_probe_sgd */
int vtx_probe_sgd(float* w, float* b, float* mw, float* mb, const float* dw, const float* db, void* shadow, const float* lr,
                  const float* wd, float mu, int H, int C, int D, void* stream) {
  if (!w || !b || !mw || !mb || !dw || !db || !lr || !wd) return VTX_ERR_NULL;
  if (H < 1 || H > PROBE_MAX_H || C < 1 || D < 1 || D > PROBE_MAX_D || (int64_t)H * C * D >= (1ll << 31)) return VTX_ERR_SHAPE;
  if (!(mu >= 0.f) || !(mu < 1.f)) return VTX_ERR_SHAPE;
  ProbeRates r;
  for (int i = 0; i < PROBE_MAX_H; ++i) {
    r.lr[i] = i < H ? lr[i] : 0.f;
    r.wd[i] = i < H ? wd[i] : 0.f;
    if (i < H && (!(lr[i] >= 0.f) || !(wd[i] >= 0.f) || !(lr[i] < INFINITY) || !(wd[i] < INFINITY))) return VTX_ERR_SHAPE;
  }
  if (D % 8 != 0) return VTX_ERR_ALIGN;
  int64_t nb = ((int64_t)C * D + C + 255) / 256;
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(probe_sgd_kernel, dim3((unsigned)nb, (unsigned)H), dim3(256), 0, (hipStream_t)stream, w, b, mw, mb, dw, db,
                     (bf16*)shadow, r, mu, C, D);
  return vtx_check_launch();
}

}  // extern "C"
