// Max-pool 3x3/s2 (resnet.py:82,190) and bilinear align_corners=True resize (aspp.py:109,
// decoder.py:34-36, deeplab.py:44,55) on NHWC fp32, forward and backward.  HBM-bound; float4 over
// channels; backward passes are written in gather form (one thread owns an input element), so they
// need no atomics and are deterministic.
#include <cmath>
#include <cstdint>
#include "common.h"
#include "zs3hip.h"

namespace {

template <typename T = float>   // element type of x and out
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* x_, int ldx, float* out_, int ldo,
                                                         unsigned char* idx, int N, int H, int W, int Ho, int Wo, int C,
                                                         int K, int stride, int pad) {
  const T* const x = reinterpret_cast<const T*>(x_);
  T* const out = reinterpret_cast<T*>(out_);
  const int c4n = C >> 2;
  const long total = (long)N * Ho * Wo * c4n;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cq = (int)(i % c4n) * 4;
    long m = i / c4n;
    const int ow = (int)(m % Wo);
    long r = m / Wo;
    const int oh = (int)(r % Ho), n = (int)(r / Ho);
    f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int bi[4] = {0, 0, 0, 0};
    for (int kh = 0; kh < K; ++kh) {
      const int h = oh * stride - pad + kh;
      if (h < 0 || h >= H) continue;
      for (int kw = 0; kw < K; ++kw) {
        const int w = ow * stride - pad + kw;
        if (w < 0 || w >= W) continue;
        f32x4 v = ld4<T>(x + (((long)n * H + h) * W + w) * ldx + cq);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (v[k] > best[k] || v[k] != v[k]) {  // first maximum wins, NaN propagates (ATen semantics)
            best[k] = v[k];
            bi[k] = kh * K + kw;
          }
      }
    }
    st4<T>(out + m * ldo + cq, best);
    if (idx) {
      unsigned pk = (unsigned)bi[0] | ((unsigned)bi[1] << 8) | ((unsigned)bi[2] << 16) | ((unsigned)bi[3] << 24);
      *reinterpret_cast<unsigned*>(idx + m * C + cq) = pk;
    }
  }
}

template <typename T = float>   // element type of dy and dx
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* dy_, int ldd, const unsigned char* idx, float* dx_,
                                                         int ldo, int N, int H, int W, int Ho, int Wo, int C, int K,
                                                         int stride, int pad) {
  const T* const dy = reinterpret_cast<const T*>(dy_);
  T* const dx = reinterpret_cast<T*>(dx_);
  const int c4n = C >> 2;
  const long total = (long)N * H * W * c4n;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cq = (int)(i % c4n) * 4;
    long m = i / c4n;
    const int w = (int)(m % W);
    long r = m / W;
    const int h = (int)(r % H), n = (int)(r / H);
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    for (int kh = 0; kh < K; ++kh) {
      const int th = h + pad - kh;
      if (th < 0 || th % stride) continue;
      const int oh = th / stride;
      if (oh >= Ho) continue;
      for (int kw = 0; kw < K; ++kw) {
        const int tw = w + pad - kw;
        if (tw < 0 || tw % stride) continue;
        const int ow = tw / stride;
        if (ow >= Wo) continue;
        const long mo = ((long)n * Ho + oh) * Wo + ow;
        const unsigned pk = *reinterpret_cast<const unsigned*>(idx + mo * C + cq);
        const f32x4 d = ld4<T>(dy + mo * ldd + cq);
        const unsigned tap = (unsigned)(kh * K + kw);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (((pk >> (8 * k)) & 0xFFu) == tap) g[k] += d[k];
      }
    }
    st4<T>(dx + m * ldo + cq, g);
  }
}

__device__ __forceinline__ void src_index(int o, float scale, int in, int& i0, int& i1, float& lam) {
  const float s = scale * (float)o;  // align_corners=True: src = dst * (in-1)/(out-1), all in fp32 as ATen does
  i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  lam = s - (float)i0;
}

// one bilinear sample; explicit FMA chain so that bilinear_fwd_kernel and the fused upsample+argmax kernel round identically
__device__ __forceinline__ float bilerp(float w00, float w01, float w10, float w11, float a, float b, float c, float d) {
  return fmaf(w11, d, fmaf(w10, c, fmaf(w01, b, w00 * a)));
}

struct ResizeArgs {
  const float* x;
  float* out;
  int N, H, W, Ho, Wo, C, ldx, ldo, accumulate;
  float sh, sw;
};

// One workgroup row (blockIdx.y) per output row (n, oh): the vertical source rows and weights are wave-uniform scalars, and a thread
// finds its (ow, channel group) with ONE 32-bit division.  (Rounds 1-3 flattened everything into one 64-bit index: three 64-bit
// divisions per element made the 21-channel upsample of the class scores -- 88 M elements, the scalar path -- ALU-bound at
// 1.0 TB/s, 346 us per step.)
template <typename T = float>   // element type of x and out
__global__ __launch_bounds__(256) void bilinear_fwd_kernel(const ResizeArgs p) {
  T* const pout = reinterpret_cast<T*>(p.out);
  const bool vec = (p.C & 3) == 0 && (p.ldx & 3) == 0 && (p.ldo & 3) == 0;
  const unsigned cn = vec ? (unsigned)(p.C >> 2) : (unsigned)p.C;
  const unsigned per_row = (unsigned)p.Wo * cn;
  for (unsigned row = blockIdx.y; row < (unsigned)(p.N * p.Ho); row += gridDim.y) {
    const unsigned n = row / (unsigned)p.Ho, oh = row - n * (unsigned)p.Ho;
    int h0, h1;
    float lh;
    src_index((int)oh, p.sh, p.H, h0, h1, lh);
    const T* const b0 = reinterpret_cast<const T*>(p.x) + ((long)n * p.H + h0) * p.W * p.ldx;
    const T* const b1 = reinterpret_cast<const T*>(p.x) + ((long)n * p.H + h1) * p.W * p.ldx;
    T* const orow = pout + (long)row * p.Wo * p.ldo;
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < per_row; idx += gridDim.x * 256u) {
      const unsigned ow = idx / cn, ci = idx - ow * cn;
      int w0, w1;
      float lw;
      src_index((int)ow, p.sw, p.W, w0, w1, lw);
      const float w00 = (1.f - lh) * (1.f - lw), w01 = (1.f - lh) * lw, w10 = lh * (1.f - lw), w11 = lh * lw;
      if (vec) {
        const int c = (int)ci * 4;
        const f32x4 a00 = ld4<T>(b0 + (long)w0 * p.ldx + c);
        const f32x4 a01 = ld4<T>(b0 + (long)w1 * p.ldx + c);
        const f32x4 a10 = ld4<T>(b1 + (long)w0 * p.ldx + c);
        const f32x4 a11 = ld4<T>(b1 + (long)w1 * p.ldx + c);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = bilerp(w00, w01, w10, w11, a00[e], a01[e], a10[e], a11[e]);
        st4<T>(orow + (long)ow * p.ldo + c, v);
      } else {
        st1<T>(orow + (long)ow * p.ldo + ci, bilerp(w00, w01, w10, w11, ld1<T>(b0 + (long)w0 * p.ldx + ci), ld1<T>(b0 + (long)w1 * p.ldx + ci),
                                                  ld1<T>(b1 + (long)w0 * p.ldx + ci), ld1<T>(b1 + (long)w1 * p.ldx + ci)));
      }
    }
  }
}

// gather-form backward: x = grad wrt the (Ho x Wo) output, out = grad wrt the (H x W) input
__device__ __forceinline__ void cand_range(int i, float scale, int out_n, int& lo, int& hi) {
  if (scale <= 0.f) {
    lo = 0;
    hi = out_n - 1;
    return;
  }
  lo = (int)floorf((float)(i - 1) / scale) - 1;
  hi = (int)ceilf((float)(i + 1) / scale) + 1;
  if (lo < 0) lo = 0;
  if (hi > out_n - 1) hi = out_n - 1;
}

// The candidate window of cand_range is conservative (11 x 11 at the 4x upsample, 7 x 7 of them with a non-zero weight): the
// column weights are computed once per input pixel (not once per candidate row), and rows / columns of zero weight are skipped
// before any address is formed.  BWD_MAXCAND bounds the unrolled column window; larger ratios take the general loop.
constexpr int BWD_MAXCAND = 12;
template <typename T = float>   // element type of the incoming and the produced gradient
__global__ __launch_bounds__(256) void bilinear_bwd_kernel(const ResizeArgs p) {
  const bool vec = (p.C & 3) == 0 && (p.ldx & 3) == 0 && (p.ldo & 3) == 0;
  const int cn = vec ? (p.C >> 2) : p.C;
  const long total = (long)p.N * p.H * p.W * cn;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ci = (int)(i % cn);
    long m = i / cn;
    const int w = (int)(m % p.W);
    long r = m / p.W;
    const int h = (int)(r % p.H), n = (int)(r / p.H);
    int olo, ohi, wlo, whi;
    cand_range(h, p.sh, p.Ho, olo, ohi);
    cand_range(w, p.sw, p.Wo, wlo, whi);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const T* g = reinterpret_cast<const T*>(p.x) + (long)n * p.Ho * p.Wo * p.ldx;
    if (whi - wlo < BWD_MAXCAND) {
      float wwv[BWD_MAXCAND];
#pragma unroll
      for (int j = 0; j < BWD_MAXCAND; ++j) {
        const int ow = wlo + j;
        int w0, w1;
        float lw;
        src_index(ow <= whi ? ow : whi, p.sw, p.W, w0, w1, lw);
        wwv[j] = ow <= whi ? (w0 == w ? 1.f - lw : 0.f) + (w1 == w ? lw : 0.f) : 0.f;
      }
      for (int oh = olo; oh <= ohi; ++oh) {
        int h0, h1;
        float lh;
        src_index(oh, p.sh, p.H, h0, h1, lh);
        const float wh = (h0 == h ? 1.f - lh : 0.f) + (h1 == h ? lh : 0.f);
        if (wh == 0.f) continue;
        // all candidates of the row in one burst of unbranched loads (window columns past `whi` re-read the last one; their
        // weight is zero and a select keeps them out of the sum): a load under `if (weight != 0)` is waited for before the
        // next one is issued
        const T* row = g + ((long)oh * p.Wo + wlo) * p.ldx + (vec ? ci * 4 : ci);
        const int jmax = whi - wlo;
        if (vec) {
          f32x4 v[BWD_MAXCAND];
#pragma unroll
          for (int j = 0; j < BWD_MAXCAND; ++j) v[j] = ld4<T>(row + (long)(j < jmax ? j : jmax) * p.ldx);
#pragma unroll
          for (int j = 0; j < BWD_MAXCAND; ++j)
            if (wwv[j] != 0.f) acc += (wh * wwv[j]) * v[j];
        } else {
          float v[BWD_MAXCAND];
#pragma unroll
          for (int j = 0; j < BWD_MAXCAND; ++j) v[j] = ld1<T>(row + (long)(j < jmax ? j : jmax) * p.ldx);
#pragma unroll
          for (int j = 0; j < BWD_MAXCAND; ++j)
            if (wwv[j] != 0.f) acc[0] += (wh * wwv[j]) * v[j];
        }
      }
    } else {
      for (int oh = olo; oh <= ohi; ++oh) {
        int h0, h1;
        float lh;
        src_index(oh, p.sh, p.H, h0, h1, lh);
        const float wh = (h0 == h ? 1.f - lh : 0.f) + (h1 == h ? lh : 0.f);
        if (wh == 0.f) continue;
        for (int ow = wlo; ow <= whi; ++ow) {
          int w0, w1;
          float lw;
          src_index(ow, p.sw, p.W, w0, w1, lw);
          const float ww = (w0 == w ? 1.f - lw : 0.f) + (w1 == w ? lw : 0.f);
          if (ww == 0.f) continue;
          const float wt = wh * ww;
          const T* src = g + ((long)oh * p.Wo + ow) * p.ldx;
          if (vec)
            acc += wt * ld4<T>(src + ci * 4);
          else
            acc[0] += wt * ld1<T>(src + ci);
        }
      }
    }
    if (vec) {
      T* dst = reinterpret_cast<T*>(p.out) + m * p.ldo + ci * 4;
      if (p.accumulate) acc += ld4<T>(dst);
      st4<T>(dst, acc);
    } else {
      T* dst = reinterpret_cast<T*>(p.out) + m * p.ldo + ci;
      st1<T>(dst, (p.accumulate ? ld1<T>(dst) : 0.f) + acc[0]);
    }
  }
}

inline int ew_blocks(long total) {
  long b = (total + 255) / 256;
  if (b > 16384) b = 16384;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

extern "C" int zs3_maxpool_fwd(const float* x, int ldx, float* out, int ldo, void* idx, int N, int H, int W, int Ho,
                               int Wo, int C, int K, int stride, int pad, int io, void* stream) {
  if (C % 4 || ldx % 4 || ldo % 4 || K * K > 255 || (io != 0 && io != 3)) return -1;
  if (io)
    hipLaunchKernelGGL((maxpool_fwd_kernel<bf16_t>), dim3(ew_blocks((long)N * Ho * Wo * (C / 4))), dim3(256), 0, (hipStream_t)stream,
                       x, ldx, out, ldo, (unsigned char*)idx, N, H, W, Ho, Wo, C, K, stride, pad);
  else
  hipLaunchKernelGGL((maxpool_fwd_kernel<float>), dim3(ew_blocks((long)N * Ho * Wo * (C / 4))), dim3(256), 0, (hipStream_t)stream,
                     x, ldx, out, ldo, (unsigned char*)idx, N, H, W, Ho, Wo, C, K, stride, pad);
  return ZS3_LAUNCH_CHECK();
}

extern "C" int zs3_maxpool_bwd(const float* dy, int ldd, const void* idx, float* dx, int ldo, int N, int H, int W,
                               int Ho, int Wo, int C, int K, int stride, int pad, int io, void* stream) {
  if (C % 4 || ldd % 4 || ldo % 4 || (io != 0 && io != 3)) return -1;
  if (io)
    hipLaunchKernelGGL((maxpool_bwd_kernel<bf16_t>), dim3(ew_blocks((long)N * H * W * (C / 4))), dim3(256), 0, (hipStream_t)stream,
                       dy, ldd, (const unsigned char*)idx, dx, ldo, N, H, W, Ho, Wo, C, K, stride, pad);
  else
  hipLaunchKernelGGL((maxpool_bwd_kernel<float>), dim3(ew_blocks((long)N * H * W * (C / 4))), dim3(256), 0, (hipStream_t)stream,
                     dy, ldd, (const unsigned char*)idx, dx, ldo, N, H, W, Ho, Wo, C, K, stride, pad);
  return ZS3_LAUNCH_CHECK();
}

// Validation (train_pascal.py:130-134 + metrics.py:73-82) without the [B,C,H,W] logits ever leaving the GPU -- or, for
// low-resolution logits, ever existing: per output pixel the C class scores are bilinearly sampled from x [N,H,W,C]
// (align_corners=True, the arithmetic of bilinear_fwd_kernel; H == Ho samples exactly), the first maximum is the
// prediction (numpy argmax), and conf[gt*C + pred] is counted for 0 <= gt < C.  Per-block LDS histogram, then integer
// atomics: the result is exact and order-independent.
template <typename T>
__global__ __launch_bounds__(256) void argmax_confusion_kernel(const ResizeArgs p, const T* target,
                                                              unsigned long long* conf) {
  extern __shared__ unsigned hist[];
  const int nbin = p.C * p.C;
  for (int i = threadIdx.x; i < nbin; i += 256) hist[i] = 0u;
  __syncthreads();
  const long total = (long)p.N * p.Ho * p.Wo;
  for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < total; m += (long)gridDim.x * blockDim.x) {
    const double gtd = (double)target[m];
    if (!(gtd >= 0.0 && gtd < (double)p.C)) continue;
    const int gt = (int)gtd;   // astype(int) truncation of metrics.py:75
    const int ow = (int)(m % p.Wo);
    const long r = m / p.Wo;
    const int oh = (int)(r % p.Ho), n = (int)(r / p.Ho);
    int h0, h1, w0, w1;
    float lh, lw;
    src_index(oh, p.sh, p.H, h0, h1, lh);
    src_index(ow, p.sw, p.W, w0, w1, lw);
    const float* b = p.x + (long)n * p.H * p.W * p.ldx;
    const float* q00 = b + ((long)h0 * p.W + w0) * p.ldx;
    const float* q01 = b + ((long)h0 * p.W + w1) * p.ldx;
    const float* q10 = b + ((long)h1 * p.W + w0) * p.ldx;
    const float* q11 = b + ((long)h1 * p.W + w1) * p.ldx;
    const float w00 = (1.f - lh) * (1.f - lw), w01 = (1.f - lh) * lw, w10 = lh * (1.f - lw), w11 = lh * lw;
    int best = 0;
    float bv = bilerp(w00, w01, w10, w11, q00[0], q01[0], q10[0], q11[0]);
    for (int c = 1; c < p.C; ++c) {
      const float v = bilerp(w00, w01, w10, w11, q00[c], q01[c], q10[c], q11[c]);
      if (v > bv) {
        bv = v;
        best = c;
      }
    }
    atomicAdd(&hist[gt * p.C + best], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nbin; i += 256)
    if (hist[i]) atomicAdd(&conf[i], (unsigned long long)hist[i]);
}

static ResizeArgs make_resize(const float* x, int ldx, float* out, int ldo, int N, int H, int W, int Ho, int Wo, int C,
                              int accumulate) {
  ResizeArgs a;
  a.x = x; a.out = out; a.N = N; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.C = C; a.ldx = ldx; a.ldo = ldo;
  a.accumulate = accumulate;
  a.sh = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f;
  a.sw = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
  return a;
}

/* x: [N,H,W,C] -> out: [N,Ho,Wo,C] */
extern "C" int zs3_bilinear_fwd(const float* x, int ldx, float* out, int ldo, int N, int H, int W, int Ho, int Wo,
                                int C, int io, void* stream) {
  if (io != 0 && io != 3) return -1;
  ResizeArgs a = make_resize(x, ldx, out, ldo, N, H, W, Ho, Wo, C, 0);
  if ((long)N * Ho <= 0 || Wo <= 0 || C <= 0) return 0;
  const long per_row = (long)Wo * ((C % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0) ? C / 4 : C);
  if (per_row >= (1L << 31) || (long)N * Ho >= (1L << 31)) return -1;
  const long rows = (long)N * Ho;
  const dim3 grid((unsigned)((per_row + 255) / 256 > 64 ? 64 : (per_row + 255) / 256), (unsigned)(rows > 4096 ? 4096 : rows));   // (rows beyond the grid: the kernel's row loop)
  if (io) hipLaunchKernelGGL((bilinear_fwd_kernel<bf16_t>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((bilinear_fwd_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, a);
  return ZS3_LAUNCH_CHECK();
}

/* dout: [N,Ho,Wo,C] (grad of the resized map) -> dx: [N,H,W,C] */
extern "C" int zs3_bilinear_bwd(const float* dout, int ldd, float* dx, int ldo, int N, int H, int W, int Ho, int Wo,
                                int C, int accumulate, int io, void* stream) {
  if (io != 0 && io != 3) return -1;
  ResizeArgs a = make_resize(dout, ldd, dx, ldo, N, H, W, Ho, Wo, C, accumulate);
  long total = (long)N * H * W * ((C % 4 == 0 && ldd % 4 == 0 && ldo % 4 == 0) ? C / 4 : C);
  if (io) hipLaunchKernelGGL((bilinear_bwd_kernel<bf16_t>), dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((bilinear_bwd_kernel<float>), dim3(ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, a);
  return ZS3_LAUNCH_CHECK();
}

/* conf[gt][pred] += 1 over all N*Ho*Wo target pixels with 0 <= gt < C; pred = argmax_c of x [N,H,W,C] bilinearly
 * resized (align_corners=True) to Ho x Wo.  conf: C*C int64 counters (caller zeroes them). */
extern "C" int zs3_argmax_confusion(const float* x, int ldx, int N, int H, int W, int C, const void* target,
                                    int target_is_i64, int Ho, int Wo, void* conf, void* stream) {
  if (C < 1 || C > 128 || N < 1) return -1;
  ResizeArgs a = make_resize(x, ldx, nullptr, 0, N, H, W, Ho, Wo, C, 0);
  const long total = (long)N * Ho * Wo;
  long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  const size_t lds = (size_t)C * C * sizeof(unsigned);
  if (target_is_i64)
    hipLaunchKernelGGL(argmax_confusion_kernel<long>, dim3((int)blocks), dim3(256), lds, (hipStream_t)stream, a,
                       (const long*)target, (unsigned long long*)conf);
  else
    hipLaunchKernelGGL(argmax_confusion_kernel<float>, dim3((int)blocks), dim3(256), lds, (hipStream_t)stream, a,
                       (const float*)target, (unsigned long long*)conf);
  return ZS3_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------ fused validation step
// Trainer.validation's per-batch tail (train_pascal.py:125-134, train_pascal_GMMN.py:337-375) from the LOW-resolution class
// scores in one pass: per target pixel the C scores are sampled with src_index / bilerp (the values zs3_bilinear_fwd would
// store), and from them come the confusion count of argmax_confusion_kernel, the weighted-CE terms of ce_tile_kernel
// (loss.hip: fp32 max / expf sum / logf, products accumulated in double) and the per-image class pixel counts.  The
// [N, Ho, Wo, C] logits never exist.
// A workgroup owns VT_H x VT_W target pixels at a time (one per thread) and stages the source patch those pixels sample --
// (8/4 + 2) x (32/4 + 2) pixels at the x4 ratio -- in LDS once, pixel stride C | 1 (odd: conflict-free across source pixels);
// each thread then walks the classes three times over LDS (argmax + max, exp sum, the target's score) instead of keeping C
// values in registers.  A tile whose patch does not fit (large C at ratio 1, downsampling) reads global memory directly.
// Tiles are dealt to blocks in contiguous runs, so a block changes image at most a few times: the class counts of an image
// are flushed when it does.  Loss sums: one (sum w*nll, sum w) pair of doubles per block, reduced in a fixed order by
// val_finalize_kernel -- no floating-point atomics, bit-reproducible.
constexpr int VT_H = 8, VT_W = 32;
constexpr int VAL_MAX_BLOCKS = 2048;

struct ValArgs {
  ResizeArgs r;
  const float* weight;
  unsigned long long* conf;
  int* class_pixels;
  double* partial;
  int ignore_index, patch_cap;   // patch_cap: floats of LDS behind the histograms (0 = never stage)
  int tiles_h, tiles_w, tiles, tiles_per_block;
};

// the C sampled scores of one pixel -> first argmax, and for a pixel the criterion counts its nll
template <bool CE>
__device__ __forceinline__ void val_pixel(const float* q00, const float* q01, const float* q10, const float* q11, float w00,
                                          float w01, float w10, float w11, int C, int t, int& best, float& nll) {
  best = 0;
  float bv = bilerp(w00, w01, w10, w11, q00[0], q01[0], q10[0], q11[0]);
  float mx = bv;
  for (int c = 1; c < C; ++c) {
    const float v = bilerp(w00, w01, w10, w11, q00[c], q01[c], q10[c], q11[c]);
    if (v > bv) {
      bv = v;
      best = c;
    }
    mx = fmaxf(mx, v);
  }
  if (CE) {
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(bilerp(w00, w01, w10, w11, q00[c], q01[c], q10[c], q11[c]) - mx);
    const float zt = bilerp(w00, w01, w10, w11, q00[t], q01[t], q10[t], q11[t]);
    nll = (mx + logf(se)) - zt;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void val_ce_confusion_kernel(const ValArgs a, const T* target) {
  extern __shared__ unsigned val_lds[];
  const ResizeArgs& p = a.r;
  const int C = p.C, nbin = C * C, CP = C | 1;
  unsigned* const hist = val_lds;                                  // [C*C] confusion counts of this block
  unsigned* const cls = val_lds + nbin;                            // [C] class pixel counts of the current image
  float* const patch = reinterpret_cast<float*>(val_lds + nbin + C);
  for (int i = threadIdx.x; i < nbin + C; i += 256) val_lds[i] = 0u;
  __syncthreads();
  const int t0 = blockIdx.x * a.tiles_per_block;
  const int t1 = min(t0 + a.tiles_per_block, a.tiles);
  const int per_img = a.tiles_h * a.tiles_w;
  const int ty = threadIdx.x / VT_W, tx = threadIdx.x % VT_W;
  double lsum = 0.0, wsum = 0.0;
  int cur_n = t0 < t1 ? t0 / per_img : 0;
  for (int tile = t0; tile < t1; ++tile) {
    const int n = tile / per_img, rem = tile - n * per_img;
    const int r0 = (rem / a.tiles_w) * VT_H, c0 = (rem % a.tiles_w) * VT_W;
    if (n != cur_n) {   // (block-uniform) the block moves on to another image: hand in the counts of the one it leaves
      __syncthreads();
      if (a.class_pixels)
        for (int i = threadIdx.x; i < C; i += 256)
          if (cls[i]) atomicAdd(&a.class_pixels[cur_n * C + i], (int)cls[i]);
      __syncthreads();
      for (int i = threadIdx.x; i < C; i += 256) cls[i] = 0u;
      cur_n = n;
    }
    // source patch of the tile: rows [ph0, ph1], columns [pw0, pw1] (src_index is monotone in the target coordinate)
    int ph0, ph1, pw0, pw1, tmp;
    float ftmp;
    src_index(r0, p.sh, p.H, ph0, tmp, ftmp);
    src_index(min(r0 + VT_H, p.Ho) - 1, p.sh, p.H, tmp, ph1, ftmp);
    src_index(c0, p.sw, p.W, pw0, tmp, ftmp);
    src_index(min(c0 + VT_W, p.Wo) - 1, p.sw, p.W, tmp, pw1, ftmp);
    const int ph = ph1 - ph0 + 1, pw = pw1 - pw0 + 1;
    const bool staged = (long)ph * pw * CP <= (long)a.patch_cap;
    const float* const img = p.x + (long)n * p.H * p.W * p.ldx;
    __syncthreads();   // the previous tile's readers are done with the patch (and the cls reset above is visible)
    if (staged) {
      const int rowf = pw * C;
      for (int e = threadIdx.x; e < ph * rowf; e += 256) {
        const int r = e / rowf, j = e - r * rowf, px = j / C, c = j - px * C;
        patch[(r * pw + px) * CP + c] = img[((long)(ph0 + r) * p.W + pw0 + px) * p.ldx + c];
      }
      __syncthreads();
    }
    const int oh = r0 + ty, ow = c0 + tx;
    if (oh < p.Ho && ow < p.Wo) {
      const long m = ((long)n * p.Ho + oh) * p.Wo + ow;
      const T tv = target[m];
      const double gtd = (double)tv;                       // the evaluator's reading of a label (argmax_confusion_kernel)
      const bool counted = gtd >= 0.0 && gtd < (double)C;
      const int t = (int)(long)tv;                         // the criterion's (loss.hip: load_target)
      const bool valid = !(t == a.ignore_index || t < 0 || t >= C);
      if (counted || valid) {
        int h0, h1, w0, w1;
        float lh, lw;
        src_index(oh, p.sh, p.H, h0, h1, lh);
        src_index(ow, p.sw, p.W, w0, w1, lw);
        const float w00 = (1.f - lh) * (1.f - lw), w01 = (1.f - lh) * lw, w10 = lh * (1.f - lw), w11 = lh * lw;
        int best;
        float nll = 0.f;
        if (staged) {
          const float* q00 = patch + ((h0 - ph0) * pw + (w0 - pw0)) * CP;
          const float* q01 = patch + ((h0 - ph0) * pw + (w1 - pw0)) * CP;
          const float* q10 = patch + ((h1 - ph0) * pw + (w0 - pw0)) * CP;
          const float* q11 = patch + ((h1 - ph0) * pw + (w1 - pw0)) * CP;
          if (valid) val_pixel<true>(q00, q01, q10, q11, w00, w01, w10, w11, C, t, best, nll);
          else val_pixel<false>(q00, q01, q10, q11, w00, w01, w10, w11, C, 0, best, nll);
        } else {
          const float* q00 = img + ((long)h0 * p.W + w0) * p.ldx;
          const float* q01 = img + ((long)h0 * p.W + w1) * p.ldx;
          const float* q10 = img + ((long)h1 * p.W + w0) * p.ldx;
          const float* q11 = img + ((long)h1 * p.W + w1) * p.ldx;
          if (valid) val_pixel<true>(q00, q01, q10, q11, w00, w01, w10, w11, C, t, best, nll);
          else val_pixel<false>(q00, q01, q10, q11, w00, w01, w10, w11, C, 0, best, nll);
        }
        if (counted) {
          const int gt = (int)gtd;   // astype(int) truncation of metrics.py:75
          atomicAdd(&hist[gt * C + best], 1u);
          atomicAdd(&cls[gt], 1u);
        }
        if (valid) {
          const float w = a.weight ? a.weight[t] : 1.f;
          lsum += (double)(w * nll);
          wsum += (double)w;
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nbin; i += 256)
    if (hist[i]) atomicAdd(&a.conf[i], (unsigned long long)hist[i]);
  if (a.class_pixels && t0 < t1)
    for (int i = threadIdx.x; i < C; i += 256)
      if (cls[i]) atomicAdd(&a.class_pixels[cur_n * C + i], (int)cls[i]);
  __shared__ double red[2][4];
  lsum = wave_sum_d(lsum);
  wsum = wave_sum_d(wsum);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = lsum;
    red[1][threadIdx.x >> 6] = wsum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.partial[2 * blockIdx.x + 0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    a.partial[2 * blockIdx.x + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

__global__ void val_zero_kernel(int* v, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) v[i] = 0;
}

// loss_ws as ce_finalize_kernel (loss.hip) leaves it, then the device-side `test_loss += loss.item()`
__global__ void val_finalize_kernel(const double* partial, int nblk, float inv_batch, float* out, double* totals) {
  double l = 0.0, w = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 64) {
    l += partial[2 * k];
    w += partial[2 * k + 1];
  }
  l = wave_sum_d(l);
  w = wave_sum_d(w);
  if (threadIdx.x == 0) {
    const float loss = (float)(l / w) * inv_batch;
    out[0] = loss;
    out[1] = (float)w;
    out[2] = (float)l;
    if (totals) {
      totals[0] += (double)loss;
      totals[1] += 1.0;
    }
  }
}

// rows (or columns) of the source a run of `span` target rows can touch: floor(scale * (span - 1)) + 1 first-rows, one more for the
// second row of the last, one more for rounding of the fp32 products -- an upper bound (the kernel checks every tile against it)
static int val_patch_extent(float scale, int span, int in) {
  const long e = (long)(scale * (float)(span - 1)) + 3;
  return (int)(e < in ? e : in);
}

extern "C" int zs3_val_ws_doubles(void) { return 2 * VAL_MAX_BLOCKS; }

extern "C" int zs3_val_ce_confusion(const float* scores, int ld, int N, int H, int W, int C, const void* target,
                                    int target_is_i64, int Ho, int Wo, const float* weight, int ignore_index, int batch,
                                    void* conf, int* class_pixels, double* partial_ws, float* loss_ws, double* totals,
                                    void* stream) {
  if (C < 1 || C > 128 || N < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || ld < C) return -1;
  if (!scores || !target || !conf || !partial_ws || !loss_ws) return -1;
  ValArgs a;
  a.r = make_resize(scores, ld, nullptr, 0, N, H, W, Ho, Wo, C, 0);
  a.weight = weight;
  a.conf = (unsigned long long*)conf;
  a.class_pixels = class_pixels;
  a.partial = partial_ws;
  a.ignore_index = ignore_index;
  a.tiles_h = (Ho + VT_H - 1) / VT_H;
  a.tiles_w = (Wo + VT_W - 1) / VT_W;
  const long tiles = (long)N * a.tiles_h * a.tiles_w;
  if (tiles >= (1L << 31) || (long)N * C >= (1L << 31)) return -1;
  a.tiles = (int)tiles;
  const int blocks = (int)(tiles < VAL_MAX_BLOCKS ? tiles : VAL_MAX_BLOCKS);
  a.tiles_per_block = (int)((tiles + blocks - 1) / blocks);
  const int nblk = (int)((tiles + a.tiles_per_block - 1) / a.tiles_per_block);   // blocks that own at least one tile
  const size_t fixed = ((size_t)C * C + C) * sizeof(unsigned);
  const size_t want = (size_t)val_patch_extent(a.r.sh, VT_H, H) * val_patch_extent(a.r.sw, VT_W, W) * (C | 1) * sizeof(float);
  const size_t budget = 64 * 1024 - 128;    // (dynamic part; `red` is static)
  a.patch_cap = fixed + want <= budget ? (int)(want / sizeof(float)) : 0;
  const size_t lds = fixed + (size_t)a.patch_cap * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (lds > budget) {   // C > ~126: the histogram alone is past the default limit
    const void* fn = target_is_i64 ? reinterpret_cast<const void*>(&val_ce_confusion_kernel<long>)
                                   : reinterpret_cast<const void*>(&val_ce_confusion_kernel<float>);
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 128) != hipSuccess) return -4;
  }
  if (class_pixels) hipLaunchKernelGGL(val_zero_kernel, dim3((N * C + 255) / 256 > 64 ? 64 : (N * C + 255) / 256), dim3(256), 0, st, class_pixels, N * C);
  if (target_is_i64)
    hipLaunchKernelGGL(val_ce_confusion_kernel<long>, dim3(nblk), dim3(256), lds, st, a, (const long*)target);
  else
    hipLaunchKernelGGL(val_ce_confusion_kernel<float>, dim3(nblk), dim3(256), lds, st, a, (const float*)target);
  hipLaunchKernelGGL(val_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)partial_ws, nblk,
                     batch > 0 ? 1.f / (float)batch : 1.f, loss_ws, totals);
  return ZS3_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------ pseudo-labelling (ZS5)
// The producer of the label maps that the reference's data sets read with weak_label=True (dataloaders/datasets/pascal.py:87-98,
// sbd.py:103-111, context.py:134-142) and for which it ships no program: the model's own prediction on the pixels whose label
// is one of the `unlabelled` classes, kept where it is among the top p % most confident of its bucket -- (image, predicted
// class) or (image).  Two entry points:
//   zs3_pl_candidates  one pass over the target pixels like val_ce_confusion_kernel (same tiles, same LDS patch, same
//                      src_index / bilerp samples): per ELIGIBLE pixel the first argmax over the candidate classes and its
//                      full-softmax probability; cls_map (255 = not eligible), conf_map, per-image class counts.  A tile
//                      without an eligible pixel stages nothing, a pixel that is not eligible samples nothing.
//   zs3_pl_select      the exact k-th largest confidence of every bucket by radix select on the BIT PATTERN of conf (a
//                      non-negative float orders like its uint32 bits): four passes of 8 bits, most significant first.  A pass is
//                      a histogram kernel (block-private LDS histograms per candidate class, integer atomics into the workspace)
//                      and a per-bucket scan (one wave per bucket) that picks the digit holding rank k, narrows the prefix and
//                      the remaining rank and clears the histogram for the next pass.  k = min(m, ceil(m * p / 100)) is computed
//                      by the first scan from `count`.  The last pass writes labels / selected / threshold: a pixel is kept
//                      iff conf >= t (ties at t are all kept).  Integer counts only: the result does not depend on the launch
//                      geometry or on the order of the atomics.
struct PlArgs {
  ResizeArgs r;
  unsigned long long cand_lo, cand_hi, unl_lo, unl_hi;
  unsigned char* cls_map;
  float* conf_map;
  int* count;
  int unl_value, ignore_index, patch_cap;   // unl_value < 0: none
  int tiles_h, tiles_w, tiles, tiles_per_block;
};

__device__ __forceinline__ bool pl_in_mask(unsigned long long lo, unsigned long long hi, int c) {
  return c >= 0 && c < 128 && (((c < 64 ? lo : hi) >> (c & 63)) & 1ull);
}
// rank of class c among the set bits of the mask
__device__ __forceinline__ int pl_slot(unsigned long long lo, unsigned long long hi, int c) {
  return c < 64 ? __popcll(lo & ((1ull << c) - 1ull)) : __popcll(lo) + __popcll(hi & ((1ull << (c - 64)) - 1ull));
}

// the C sampled scores of one pixel -> first argmax over the candidate classes and its probability under the softmax over
// ALL classes (fp32, the arithmetic of val_pixel: max, expf sum)
__device__ __forceinline__ void pl_pixel(const float* q00, const float* q01, const float* q10, const float* q11, float w00,
                                         float w01, float w10, float w11, int C, unsigned long long lo,
                                         unsigned long long hi, int& best, float& conf) {
  best = -1;
  float bv = 0.f, mx = bilerp(w00, w01, w10, w11, q00[0], q01[0], q10[0], q11[0]);
  for (int c = 0; c < C; ++c) {
    const float v = bilerp(w00, w01, w10, w11, q00[c], q01[c], q10[c], q11[c]);
    mx = fmaxf(mx, v);
    if (pl_in_mask(lo, hi, c) && (best < 0 || v > bv)) {
      bv = v;
      best = c;
    }
  }
  float se = 0.f;
  for (int c = 0; c < C; ++c) se += expf(bilerp(w00, w01, w10, w11, q00[c], q01[c], q10[c], q11[c]) - mx);
  conf = expf(bv - mx) / se;
}

template <typename T>
__global__ __launch_bounds__(256) void pl_candidates_kernel(const PlArgs a, const T* target) {
  extern __shared__ unsigned pl_lds[];
  const ResizeArgs& p = a.r;
  const int C = p.C, CP = C | 1;
  unsigned* const cls = pl_lds;                                     // [C] eligible pixels per predicted class, current image
  float* const patch = reinterpret_cast<float*>(pl_lds + C);
  for (int i = threadIdx.x; i < C; i += 256) cls[i] = 0u;
  const int t0 = blockIdx.x * a.tiles_per_block;
  const int t1 = min(t0 + a.tiles_per_block, a.tiles);
  const int per_img = a.tiles_h * a.tiles_w;
  const int ty = threadIdx.x / VT_W, tx = threadIdx.x % VT_W;
  int cur_n = t0 < t1 ? t0 / per_img : 0;
  for (int tile = t0; tile < t1; ++tile) {
    const int n = tile / per_img, rem = tile - n * per_img;
    const int r0 = (rem / a.tiles_w) * VT_H, c0 = (rem % a.tiles_w) * VT_W;
    if (n != cur_n) {   // (block-uniform) the block moves on to another image: hand in the counts of the one it leaves
      __syncthreads();
      for (int i = threadIdx.x; i < C; i += 256)
        if (cls[i]) atomicAdd(&a.count[cur_n * C + i], (int)cls[i]);
      __syncthreads();
      for (int i = threadIdx.x; i < C; i += 256) cls[i] = 0u;
      cur_n = n;
    }
    const int oh = r0 + ty, ow = c0 + tx;
    const bool inside = oh < p.Ho && ow < p.Wo;
    const long m = ((long)n * p.Ho + oh) * p.Wo + ow;
    bool eligible = false;
    if (inside) {
      const int t = (int)(long)target[m];                  // the criterion's reading of a label (loss.hip: load_target)
      eligible = t != a.ignore_index && (pl_in_mask(a.unl_lo, a.unl_hi, t) || (a.unl_value >= 0 && t == a.unl_value));
    }
    // (a barrier as well: the previous tile's readers are done with the patch, the cls reset above is visible)
    const bool any = __syncthreads_or(eligible);
    if (!any) {   // (block-uniform) nothing to label in this tile
      if (inside) {
        a.cls_map[m] = 255;
        a.conf_map[m] = 0.f;
      }
      continue;
    }
    int ph0, ph1, pw0, pw1, tmp;
    float ftmp;
    src_index(r0, p.sh, p.H, ph0, tmp, ftmp);
    src_index(min(r0 + VT_H, p.Ho) - 1, p.sh, p.H, tmp, ph1, ftmp);
    src_index(c0, p.sw, p.W, pw0, tmp, ftmp);
    src_index(min(c0 + VT_W, p.Wo) - 1, p.sw, p.W, tmp, pw1, ftmp);
    const int ph = ph1 - ph0 + 1, pw = pw1 - pw0 + 1;
    const bool staged = (long)ph * pw * CP <= (long)a.patch_cap;
    const float* const img = p.x + (long)n * p.H * p.W * p.ldx;
    if (staged) {
      const int rowf = pw * C;
      for (int e = threadIdx.x; e < ph * rowf; e += 256) {
        const int r = e / rowf, j = e - r * rowf, px = j / C, c = j - px * C;
        patch[(r * pw + px) * CP + c] = img[((long)(ph0 + r) * p.W + pw0 + px) * p.ldx + c];
      }
      __syncthreads();
    }
    if (!inside) continue;
    int best = 255;
    float conf = 0.f;
    if (eligible) {
      int h0, h1, w0, w1;
      float lh, lw;
      src_index(oh, p.sh, p.H, h0, h1, lh);
      src_index(ow, p.sw, p.W, w0, w1, lw);
      const float w00 = (1.f - lh) * (1.f - lw), w01 = (1.f - lh) * lw, w10 = lh * (1.f - lw), w11 = lh * lw;
      if (staged) {
        const float* q00 = patch + ((h0 - ph0) * pw + (w0 - pw0)) * CP;
        const float* q01 = patch + ((h0 - ph0) * pw + (w1 - pw0)) * CP;
        const float* q10 = patch + ((h1 - ph0) * pw + (w0 - pw0)) * CP;
        const float* q11 = patch + ((h1 - ph0) * pw + (w1 - pw0)) * CP;
        pl_pixel(q00, q01, q10, q11, w00, w01, w10, w11, C, a.cand_lo, a.cand_hi, best, conf);
      } else {
        const float* q00 = img + ((long)h0 * p.W + w0) * p.ldx;
        const float* q01 = img + ((long)h0 * p.W + w1) * p.ldx;
        const float* q10 = img + ((long)h1 * p.W + w0) * p.ldx;
        const float* q11 = img + ((long)h1 * p.W + w1) * p.ldx;
        pl_pixel(q00, q01, q10, q11, w00, w01, w10, w11, C, a.cand_lo, a.cand_hi, best, conf);
      }
      atomicAdd(&cls[best], 1u);
    }
    a.cls_map[m] = (unsigned char)best;
    a.conf_map[m] = conf;
  }
  __syncthreads();
  if (t0 < t1)
    for (int i = threadIdx.x; i < C; i += 256)
      if (cls[i]) atomicAdd(&a.count[cur_n * C + i], (int)cls[i]);
}

// the candidate mask names at least one class and none at or beyond C
static bool pl_mask_ok(unsigned long long lo, unsigned long long hi, int C) {
  if (!(lo | hi)) return false;
  if (C < 64) return !hi && !(lo >> C);
  return C == 128 || !(hi >> (C - 64));
}

extern "C" int zs3_pl_candidates(const float* scores, int ld, int N, int H, int W, int C, const void* target,
                                 int target_is_i64, int Ho, int Wo, unsigned long long cand_lo, unsigned long long cand_hi,
                                 unsigned long long unl_lo, unsigned long long unl_hi, int unlabelled_value,
                                 int ignore_index, unsigned char* cls_map, float* conf_map, int* count, void* stream) {
  if (C < 1 || C > 128 || N < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || ld < C) return -1;
  if (!scores || !target || !cls_map || !conf_map || !count || !pl_mask_ok(cand_lo, cand_hi, C)) return -1;
  PlArgs a;
  a.r = make_resize(scores, ld, nullptr, 0, N, H, W, Ho, Wo, C, 0);
  a.cand_lo = cand_lo; a.cand_hi = cand_hi; a.unl_lo = unl_lo; a.unl_hi = unl_hi;
  a.cls_map = cls_map; a.conf_map = conf_map; a.count = count;
  a.unl_value = unlabelled_value;
  a.ignore_index = ignore_index;
  a.tiles_h = (Ho + VT_H - 1) / VT_H;
  a.tiles_w = (Wo + VT_W - 1) / VT_W;
  const long tiles = (long)N * a.tiles_h * a.tiles_w;
  if (tiles >= (1L << 31) || (long)N * C >= (1L << 31)) return -1;
  a.tiles = (int)tiles;
  const int blocks = (int)(tiles < 4 * VAL_MAX_BLOCKS ? tiles : 4 * VAL_MAX_BLOCKS);
  a.tiles_per_block = (int)((tiles + blocks - 1) / blocks);
  const int nblk = (int)((tiles + a.tiles_per_block - 1) / a.tiles_per_block);
  const size_t fixed = (size_t)C * sizeof(unsigned);
  const size_t want = (size_t)val_patch_extent(a.r.sh, VT_H, H) * val_patch_extent(a.r.sw, VT_W, W) * (C | 1) * sizeof(float);
  const size_t budget = 64 * 1024 - 128;
  a.patch_cap = fixed + want <= budget ? (int)(want / sizeof(float)) : 0;
  const size_t lds = fixed + (size_t)a.patch_cap * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(val_zero_kernel, dim3((N * C + 255) / 256 > 64 ? 64 : (N * C + 255) / 256), dim3(256), 0, st, count, N * C);
  if (target_is_i64)
    hipLaunchKernelGGL(pl_candidates_kernel<long>, dim3(nblk), dim3(256), lds, st, a, (const long*)target);
  else
    hipLaunchKernelGGL(pl_candidates_kernel<float>, dim3(nblk), dim3(256), lds, st, a, (const float*)target);
  return ZS3_LAUNCH_CHECK();
}

// ---- selection
constexpr int PL_BINS = 256, PL_PASSES = 4;   // 8-bit digits of the 32-bit pattern, most significant first

struct PlSel {
  const unsigned* conf;          // conf_map read as bit patterns (no arithmetic touches it: denormals stay what they are)
  const unsigned char* cls;
  const int* count;
  unsigned* hist;                // workspace: [buckets][PL_BINS]
  unsigned* prefix;              // [buckets] the bits of t settled so far (right-aligned)
  unsigned* krem;                // [buckets] the rank still to be found inside the prefix; 0: the bucket keeps nothing
  unsigned long long cand_lo, cand_hi;
  int N, C, P;                   // P: pixels per image
  int group;                     // 0: bucket = (image, class), index n*C + c;  1: bucket = image, index n
  int pass, shift, nslots, lds_hist, per_block;
  double top_percent;
};

// per class of image n: the bucket's prefix and remaining rank, and the row of the block's LDS histogram
__device__ __forceinline__ void pl_load_buckets(const PlSel& a, int n, unsigned* pre, unsigned* rank, int* slot) {
  for (int c = threadIdx.x; c < a.C; c += blockDim.x) {
    const bool is_cand = pl_in_mask(a.cand_lo, a.cand_hi, c);
    const int b = a.group ? n : n * a.C + c;
    pre[c] = is_cand ? a.prefix[b] : 0u;
    rank[c] = is_cand ? a.krem[b] : 0u;
    slot[c] = !is_cand ? -1 : (a.group ? 0 : pl_slot(a.cand_lo, a.cand_hi, c));
  }
}

__global__ __launch_bounds__(256) void pl_hist_kernel(const PlSel a) {
  extern __shared__ unsigned pl_hist_lds[];      // [nslots][PL_BINS] when lds_hist
  __shared__ unsigned pre[128], rank[128];
  __shared__ int slot[128], slot_cls[128];
  const int n = blockIdx.y;
  pl_load_buckets(a, n, pre, rank, slot);
  if (a.lds_hist)
    for (int i = threadIdx.x; i < a.nslots * PL_BINS; i += 256) pl_hist_lds[i] = 0u;
  __syncthreads();
  for (int c = threadIdx.x; c < a.C; c += 256)
    if (slot[c] >= 0 && !a.group) slot_cls[slot[c]] = c;
  const long base = (long)n * a.P;
  const int i0 = blockIdx.x * a.per_block, i1 = min(i0 + a.per_block, a.P);
  for (int i = i0 + threadIdx.x; i < i1; i += 256) {
    const int c = a.cls[base + i];
    if (c >= a.C) continue;                       // 255: not eligible
    const int s = slot[c];
    if (s < 0) continue;
    const unsigned bits = a.conf[base + i];
    if (a.pass > 0 && (rank[c] == 0u || (bits >> (a.shift + 8)) != pre[c])) continue;
    const unsigned d = (bits >> a.shift) & (PL_BINS - 1);
    if (a.lds_hist) atomicAdd(&pl_hist_lds[s * PL_BINS + d], 1u);
    else atomicAdd(&a.hist[(long)(a.group ? n : n * a.C + c) * PL_BINS + d], 1u);
  }
  if (!a.lds_hist) return;
  __syncthreads();
  for (int i = threadIdx.x; i < a.nslots * PL_BINS; i += 256) {
    const unsigned v = pl_hist_lds[i];
    if (v) atomicAdd(&a.hist[(long)(a.group ? n : n * a.C + slot_cls[i / PL_BINS]) * PL_BINS + (i % PL_BINS)], v);
  }
}

// one wave per bucket: lane l owns bins 4l .. 4l+3.  Finds the digit d with #{bins > d} < k <= #{bins >= d}, appends it to the
// prefix, takes #{bins > d} off the rank and clears the histogram.  Pass 0 computes k; the last pass writes the threshold.
__global__ __launch_bounds__(64) void pl_scan_kernel(const PlSel a, unsigned* threshold) {
  __shared__ unsigned found[2];
  const int b = blockIdx.x, lane = threadIdx.x;
  u32x4* const h = reinterpret_cast<u32x4*>(a.hist + (long)b * PL_BINS);
  const u32x4 v = h[lane];
  h[lane] = u32x4{0u, 0u, 0u, 0u};
  unsigned k;
  if (a.pass == 0) {
    int m = 0;
    if (a.group) {
      for (int c = lane; c < a.C; c += 64) m += a.count[b * a.C + c];
      for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
    } else {
      m = a.count[b];
    }
    const double want = ceil((double)m * a.top_percent / 100.0);
    k = (unsigned)(want < (double)m ? want : (double)m);
  } else {
    k = a.krem[b];
  }
  if (lane == 0) {
    found[0] = a.pass == 0 ? 0u : a.prefix[b];
    found[1] = 0u;
  }
  __syncthreads();
  if (k > 0u) {
    const unsigned own = v[0] + v[1] + v[2] + v[3];
    unsigned incl = own;   // sum over lanes >= this one
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t = __shfl_down(incl, o, 64);
      if (lane + o < 64) incl += t;
    }
    unsigned above = incl - own;
    if (above < k && k <= incl) {   // exactly one lane (1 <= k <= number of values counted)
      int d = 3;
      while (above + v[d] < k) {
        above += v[d];
        --d;
      }
      found[0] = ((a.pass == 0 ? 0u : a.prefix[b]) << 8) | (unsigned)(4 * lane + d);
      found[1] = k - above;
    }
  }
  __syncthreads();
  if (lane == 0) {
    a.prefix[b] = found[0];
    a.krem[b] = found[1];
  }
  if (a.pass == PL_PASSES - 1) {
    const unsigned t = found[1] ? found[0] : 0u;
    if (a.group) {
      for (int c = lane; c < a.C; c += 64) threshold[b * a.C + c] = pl_in_mask(a.cand_lo, a.cand_hi, c) ? t : 0u;
    } else if (lane == 0) {
      threshold[b] = t;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void pl_final_kernel(const PlSel a, const T* target, T* labels, int* selected, int ignore_index,
                                                      unsigned long long* totals) {
  __shared__ unsigned pre[128], rank[128], sel[128];
  __shared__ int slot[128];
  const int n = blockIdx.y;
  pl_load_buckets(a, n, pre, rank, slot);
  for (int c = threadIdx.x; c < 128; c += 256) sel[c] = 0u;
  __syncthreads();
  const long base = (long)n * a.P;
  const int i0 = blockIdx.x * a.per_block, i1 = min(i0 + a.per_block, a.P);
  for (int i = i0 + threadIdx.x; i < i1; i += 256) {
    const int c = a.cls[base + i];
    T out;
    if (c >= a.C) {
      out = target[base + i];
    } else {
      const bool keep = rank[c] != 0u && a.conf[base + i] >= pre[c];
      out = keep ? (T)c : (T)ignore_index;
      if (keep) atomicAdd(&sel[c], 1u);
    }
    labels[base + i] = out;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < a.C; c += 256)
    if (sel[c]) atomicAdd(&selected[n * a.C + c], (int)sel[c]);
  if (totals)   // running sums over the calls: [0][c] += count, [1][c] += selected (integers: exact in any order)
    for (int c = threadIdx.x; c < a.C; c += 256) {
      const int cnt = blockIdx.x == 0 ? a.count[n * a.C + c] : 0;
      if (cnt) atomicAdd(&totals[c], (unsigned long long)cnt);
      if (sel[c]) atomicAdd(&totals[a.C + c], (unsigned long long)sel[c]);
    }
}

__global__ void pl_clear_kernel(unsigned* ws, long nws, int* selected, int nsel) {
  const long step = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nws; i += step) ws[i] = 0u;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nsel; i += step) selected[i] = 0;
}

extern "C" long zs3_pl_ws_bytes(int N, int C) {
  if (N < 1 || C < 1 || C > 128) return -1;
  return (long)N * C * (PL_BINS + 2) * (long)sizeof(unsigned);
}

extern "C" int zs3_pl_select(const float* conf_map, const unsigned char* cls_map, const void* target, int target_is_i64,
                             int N, int Ho, int Wo, int C, unsigned long long cand_lo, unsigned long long cand_hi,
                             const int* count, double top_percent, int group, int ignore_index, void* labels,
                             int* selected, float* threshold, void* totals, void* ws, void* stream) {
  if (C < 1 || C > 128 || N < 1 || N > 65535 || Ho < 1 || Wo < 1 || (long)Ho * Wo >= (1L << 31) || (long)N * C >= (1L << 23)) return -1;
  if (!conf_map || !cls_map || !target || !count || !labels || !selected || !threshold || !ws) return -1;
  if (!pl_mask_ok(cand_lo, cand_hi, C) || (group != 0 && group != 1) || !(top_percent >= 0.0 && top_percent <= 100.0)) return -1;
  if (((uintptr_t)ws & 15u) != 0) return -1;   // (the scan reads a bucket's histogram 16 bytes per lane)
  const long nb = (long)N * C;
  PlSel a;
  a.conf = reinterpret_cast<const unsigned*>(conf_map);
  a.cls = cls_map;
  a.count = count;
  a.hist = static_cast<unsigned*>(ws);
  a.prefix = a.hist + nb * PL_BINS;
  a.krem = a.prefix + nb;
  a.cand_lo = cand_lo; a.cand_hi = cand_hi;
  a.N = N; a.C = C; a.P = Ho * Wo;
  a.group = group;
  a.nslots = group ? 1 : __builtin_popcountll(cand_lo) + __builtin_popcountll(cand_hi);
  const size_t hist_lds = (size_t)a.nslots * PL_BINS * sizeof(unsigned);
  a.lds_hist = hist_lds <= 60 * 1024;
  a.top_percent = top_percent;
  int bx = (a.P + 256 * 16 - 1) / (256 * 16);
  if (bx > 128) bx = 128;
  a.per_block = (a.P + bx - 1) / bx;
  bx = (a.P + a.per_block - 1) / a.per_block;
  const dim3 grid(bx, N);
  const int buckets = group ? N : (int)nb;
  hipStream_t st = (hipStream_t)stream;
  const long nws = nb * (PL_BINS + 2);
  hipLaunchKernelGGL(pl_clear_kernel, dim3((int)((nws + 255) / 256 > 256 ? 256 : (nws + 255) / 256)), dim3(256), 0, st,
                     a.hist, nws, selected, (int)nb);
  for (int pass = 0; pass < PL_PASSES; ++pass) {
    a.pass = pass;
    a.shift = 32 - 8 * (pass + 1);
    hipLaunchKernelGGL(pl_hist_kernel, grid, dim3(256), a.lds_hist ? hist_lds : 0, st, a);
    hipLaunchKernelGGL(pl_scan_kernel, dim3(buckets), dim3(64), 0, st, a, reinterpret_cast<unsigned*>(threshold));
  }
  if (target_is_i64)
    hipLaunchKernelGGL(pl_final_kernel<long>, grid, dim3(256), 0, st, a, (const long*)target, (long*)labels, selected, ignore_index,
                       (unsigned long long*)totals);
  else
    hipLaunchKernelGGL(pl_final_kernel<float>, grid, dim3(256), 0, st, a, (const float*)target, (float*)labels, selected, ignore_index,
                       (unsigned long long*)totals);
  return ZS3_LAUNCH_CHECK();
}
