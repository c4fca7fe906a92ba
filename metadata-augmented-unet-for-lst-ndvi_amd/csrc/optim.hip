// optim.hip -- the AdamW update of every 3x3 convolution weight of a network AND the re-pack of the updated weights, one launch.
//
// An optimizer step of the reference (torch.optim.AdamW, src/train.py:213-214,255) is followed, on this path, by re-packing all
// convolution weights into the matrix-core layouts (forward pack and data-gradient pack, conv3x3.hip).  As separate passes that is
//     AdamW:  read p, g, m, v; write p, m, v            (7 x 4 bytes per parameter)
//     pack :  read p (twice: the two packs are tiled differently); write 2 x 2 bytes
// Here one workgroup owns a 64 (output channel) x 64 (input channel) x 9 (tap) block of ONE layer: it streams the block's p, g, m, v
// once, applies AdamW, writes p, m, v back and keeps the new weights in LDS (147 KB), from which BOTH packs of the block -- four
// 16-channel chunks each, rows permuted for the 16-bit kernels exactly as pack_weights_kernel does -- are written.
//     fused:  read p, g, m, v; write p, m, v, 2 x 2 bytes        (32 bytes per parameter instead of 40, one launch instead of ~5)
// The update is torch's AdamW (decoupled weight decay, bias correction, eps outside the root):
//     p <- p (1 - lr wd);  m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2;  p <- p - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// with the step count t read from DEVICE memory (the step is capturable into a hipGraph).
//
// The same tile / LDS / pack half serves the reference's other two optimizers (src/train.py:209-212), the rule being a template parameter:
//     Adam  (torch.optim.Adam, L2 decay):  g <- g + wd p;  then the moments and the step above, without the decoupled decay
//     SGD   (torch.optim.SGD, dampening 0): g <- g + wd p;  buf <- mu buf + g;  p <- p - lr (nesterov ? g + mu buf : buf)      (mu = 0: no buffer)
// and gradient clipping (src/train.py:253-254) rides along: with a device scalar `grad_scale` every gradient is multiplied by it as it
// is loaded -- clip_grad_norm_'s pass that reads and rewrites every gradient disappears.  The scalar comes from grad_norm_clip_kernel
// below: the global L2 norm of all gradients in ONE launch (fp64 partial per workgroup, the last workgroup to take a ticket adds the
// partials in index order) and clip_coef_clamped = min(1, max_norm / (norm + 1e-6)).
#include "mau_common.h"

namespace mau {

struct AdamWPackDesc {
  float* w;
  const float* g;
  float* m;
  float* v;
  void* wf;
  void* wd;
  int Cout, Cin, nCoB, tile0;
};

constexpr int OPT_ROW = 64 * 9 + 1;      // LDS row: 64 input channels x 9 taps (+1: bank spread)

// beta1 doubles as SGD's momentum.  gscale: device scalar every gradient is multiplied by as it is loaded (NULL: none).
template <typename T, int RULE>
__global__ __launch_bounds__(1024) void opt_pack_kernel(const AdamWPackDesc* __restrict__ descs, int n, const float* __restrict__ step_ptr,
                                                        const float* __restrict__ gscale, float lr, float beta1, float beta2, float eps, float wd,
                                                        int nesterov) {
  extern __shared__ float tile[];                       // [64][OPT_ROW]: tile[co_local][ci_local * 9 + tap]
  int i = 0;
  while (i + 1 < n && (int)blockIdx.x >= descs[i + 1].tile0) ++i;
  const AdamWPackDesc d = descs[i];
  const int t = (int)blockIdx.x - d.tile0;
  const int cob = t % d.nCoB, cib = t / d.nCoB;
  const int co0 = cob * 64, ci0 = cib * 64;
  const int Cout = d.Cout, Cin = d.Cin;
  const int CoutPad = (Cout + 63) / 64 * 64, CinPad = (Cin + 63) / 64 * 64;
  const float step = RULE == MAU_OPT_SGD ? 1.f : *step_ptr;
  const float gs = gscale != nullptr ? *gscale : 1.f;
  const float bc1 = 1.f - powf(beta1, step), bc2s = sqrtf(1.f - powf(beta2, step));
  const float step_size = lr / bc1, decay = 1.f - lr * wd;
  // ---- AdamW on the block: row r = output channel co0 + r, 576 contiguous floats (64 input channels x 9 taps) of the OIHW tensor ----
  const int ncol = (Cin - ci0 < 64 ? Cin - ci0 : 64) * 9;          // valid floats of a row
  for (int e = threadIdx.x; e < 64 * 576; e += 1024) {
    const int r = e / 576, k = e - r * 576;
    float pn = 0.f;
    if (co0 + r < Cout && k < ncol) {
      const size_t idx = ((size_t)(co0 + r) * Cin + ci0) * 9 + k;
      float g = d.g[idx];
      float p = d.w[idx];
      if (gscale != nullptr) g *= gs;                        // (clipping: before the weight decay, as clip_grad_norm_ + step() would)
      if (RULE == MAU_OPT_SGD) {
        // torch's order and roundings (measured bit for bit against torch.optim.SGD on gfx950): grad.add(p, alpha=wd) and
        // p.add_(g, alpha=-lr) are one fused multiply-add each, buf.mul_(mu).add_(g) is two operations -- the product is rounded
        // (opaque() keeps the compiler from contracting it).  The rule itself -- order, buffer, nesterov term, grad_scale in front
        // of the decay -- is pinned bit for bit on inputs where no rounding occurs by tests/test_gpu_optim_pack.py::test_sgd_exact
        if (wd != 0.f) g = fmaf(wd, p, g);
        if (d.m != nullptr) {
          const float buf = opaque(beta1 * d.m[idx]) + g;
          d.m[idx] = buf;
          g = nesterov ? fmaf(beta1, buf, g) : buf;
        }
        p = fmaf(-lr, g, p);
      } else {
        float m = d.m[idx], v = d.v[idx];
        if (RULE == MAU_OPT_ADAMW) p *= decay;
        else if (wd != 0.f) g = g + wd * p;
        m = fmaf(beta1, m, (1.f - beta1) * g);                 // (lerp(m, g, 1 - b1))
        v = fmaf(beta2, v, (1.f - beta2) * g * g);
        const float denom = sqrtf(v) / bc2s + eps;
        p = p - step_size * (m / denom);
        d.m[idx] = m;
        d.v[idx] = v;
      }
      d.w[idx] = p;
      pn = p;
    }
    tile[r * OPT_ROW + k] = pn;
  }
  __syncthreads();
  if (d.wf == nullptr && d.wd == nullptr) return;
  // ---- the block's share of both packs (layouts of pack_tile, conv3x3.hip): four 16-channel chunks each ----
  // forward  wf[((chunk * 9 + tap) * CoutPad + co0 + pos) * 16 + k] = W[co0 + ch(pos)][chunk * 16 + k][tap],       chunk = ci0 / 16 + cc
  // dgrad    wd[((chunk * 9 + 8 - tap) * CinPad + ci0 + pos) * 16 + k] = W[chunk * 16 + k][ci0 + ch(pos)][tap],    chunk = co0 / 16 + cc
  // (ch(pos) = 2 (pos & 31) + (pos >> 5) for the 16-bit packs: the two accumulator tiles of an MFMA lane carry adjacent channels)
  const int nchF = (Cin + 15) / 16, nchD = (Cout + 15) / 16;
  T* wf = (T*)d.wf;
  T* wdp = (T*)d.wd;
  for (int e = threadIdx.x; e < 2 * 4 * 9 * 64 * 2; e += 1024) {
    const int k8 = e & 1, pos = (e >> 1) & 63, tap = (e >> 7) % 9, cc = ((e >> 7) / 9) & 3, which = (e >> 7) / 36;
    const int ch = sizeof(T) == 2 ? 2 * (pos & 31) + (pos >> 5) : pos;
    F8 val;
    if (which == 0) {
      const int chunk = ci0 / 16 + cc;
      if (wf == nullptr || chunk >= nchF) continue;
#pragma unroll
      for (int j = 0; j < 8; ++j) val.v[j] = tile[ch * OPT_ROW + (cc * 16 + k8 * 8 + j) * 9 + tap];
      store8<T>(wf + (((size_t)chunk * 9 + tap) * CoutPad + co0 + pos) * 16 + k8 * 8, val);
    } else {
      const int chunk = co0 / 16 + cc;
      if (wdp == nullptr || chunk >= nchD) continue;
#pragma unroll
      for (int j = 0; j < 8; ++j) val.v[j] = tile[(cc * 16 + k8 * 8 + j) * OPT_ROW + ch * 9 + tap];
      store8<T>(wdp + (((size_t)chunk * 9 + 8 - tap) * CinPad + ci0 + pos) * 16 + k8 * 8, val);
    }
  }
}

// ---- global gradient norm + clip coefficient, one launch ----
struct NormSeg {
  const float* ptr;
  int64_t n;
  int block0, pad;
};
constexpr int NORM_CHUNK = 8192;      // floats of ONE segment a workgroup sums: 256 threads x 8 x 16 bytes

// Workgroup b sums the squares of chunk (b - block0) of its segment in fp64 -- 16-byte loads from the first 16-byte-aligned element on,
// scalar loads for the few elements in front of it and behind the last whole vector; which thread adds which element depends on the
// segment's address and length only -- and publishes the partial.  The last workgroup to take the ticket adds the partials in index
// order (256 contiguous runs, then the 256 run sums): the result does not depend on the order the workgroups ran in.
__global__ __launch_bounds__(256) void grad_norm_clip_kernel(const NormSeg* __restrict__ segs, int nsegs, double* __restrict__ part,
                                                             unsigned* __restrict__ ticket, float max_norm, float* __restrict__ norm_out,
                                                             float* __restrict__ coef_out) {
  __shared__ double red[256];
  const int b = blockIdx.x, nb = gridDim.x;
  int lo = 0, hi = nsegs - 1;                              // the last segment whose block0 <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].block0 <= b) lo = mid; else hi = mid - 1;
  }
  const NormSeg sg = segs[lo];
  const int64_t e0 = (int64_t)(b - sg.block0) * NORM_CHUNK;
  const int64_t e1 = e0 + NORM_CHUNK < sg.n ? e0 + NORM_CHUNK : sg.n;
  double s = 0.0;
  if (e0 < e1) {
    const float* p = sg.ptr;
    const int mis = (int)(((uintptr_t)(p + e0) >> 2) & 3);          // (NORM_CHUNK is a multiple of 4: the same for every chunk)
    int64_t a0 = e0 + ((4 - mis) & 3);
    if (a0 > e1) a0 = e1;
    const int64_t nvec = (e1 - a0) >> 2;
    const int64_t a1 = a0 + nvec * 4;
    for (int64_t i = threadIdx.x; i < nvec; i += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p + a0 + i * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) s = fma((double)v[j], (double)v[j], s);
    }
    const int64_t head = a0 - e0, tail = e1 - a1;                    // < 4 each
    if ((int64_t)threadIdx.x < head) {
      const double x = (double)p[e0 + threadIdx.x];
      s = fma(x, x, s);
    } else if ((int64_t)threadIdx.x >= 4 && (int64_t)threadIdx.x - 4 < tail) {
      const double x = (double)p[a1 + threadIdx.x - 4];
      s = fma(x, x, s);
    }
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[b] = red[0];
  if (!last_block_of(ticket, (unsigned)nb)) return;
  const int per = (nb + 255) / 256;
  const int k0 = (int)threadIdx.x * per, k1 = k0 + per < nb ? k0 + per : nb;
  double t = 0.0;
  for (int k = k0; k < k1; ++k) t += part[k];
  red[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int k = 0; k < 256; ++k) tot += red[k];
    const float norm = (float)sqrt(tot);
    const float c = max_norm / (norm + 1e-6f);
    *norm_out = norm;
    *coef_out = c > 1.f ? 1.f : c;                         // (a NaN stays a NaN, as torch.clamp keeps it)
  }
}

}  // namespace mau

using namespace mau;

extern "C" {

size_t mau_adamw_pack_desc_bytes(void) { return sizeof(AdamWPackDesc); }

int mau_adamw_pack_desc_fill(void* descs_host, int index, float* w, const float* grad, float* exp_avg, float* exp_avg_sq, void* wf,
                             void* wd, int Cout, int Cin, int tile0, int* next_tile_host) {
  MAU_REQUIRE(exp_avg && exp_avg_sq, "adamw_pack_desc_fill: bad arguments");
  return mau_opt_pack_desc_fill(descs_host, index, w, grad, exp_avg, exp_avg_sq, wf, wd, Cout, Cin, tile0, next_tile_host);
}

int mau_opt_pack_desc_fill(void* descs_host, int index, float* w, const float* grad, float* m, float* v, void* wf, void* wd, int Cout,
                           int Cin, int tile0, int* next_tile_host) {
  MAU_REQUIRE(descs_host && next_tile_host && index >= 0 && w && grad && Cout > 0 && Cin > 0 && tile0 >= 0, "opt_pack_desc_fill: bad arguments");
  AdamWPackDesc* d = reinterpret_cast<AdamWPackDesc*>(descs_host) + index;
  d->w = w; d->g = grad; d->m = m; d->v = v; d->wf = wf; d->wd = wd; d->Cout = Cout; d->Cin = Cin;
  d->nCoB = round_up(Cout, 64) / 64; d->tile0 = tile0;
  *next_tile_host = tile0 + d->nCoB * (round_up(Cin, 64) / 64);
  return MAU_OK;
}

int mau_adamw_pack_step(const void* descs, int n, int total_tiles, int dtype, const float* step, float lr, float beta1, float beta2,
                        float eps, float weight_decay, mau_stream_t stream) {
  MAU_REQUIRE(step, "adamw_pack_step: bad arguments");
  return mau_opt_pack_step(descs, n, total_tiles, dtype, MAU_OPT_ADAMW, step, nullptr, lr, beta1, beta2, eps, weight_decay, 0, stream);
}

// (the rows of an Adam / AdamW table carry both moments, those of an SGD table a momentum buffer exactly when momentum != 0: the
//  table lives on the device, the caller answers for it as it does for every other address in it)
int mau_opt_pack_step(const void* descs, int n, int total_tiles, int dtype, int rule, const float* step, const float* grad_scale, float lr,
                      float beta1_or_momentum, float beta2, float eps, float weight_decay, int nesterov, mau_stream_t stream) {
  const float beta1 = beta1_or_momentum;
  MAU_REQUIRE(descs && n > 0 && total_tiles > 0 && lr >= 0.f && beta1 >= 0.f && eps >= 0.f, "opt_pack_step: bad arguments");
  MAU_REQUIRE(rule == MAU_OPT_ADAMW || rule == MAU_OPT_ADAM || rule == MAU_OPT_SGD, "opt_pack_step: unknown rule %d", rule);
  if (rule == MAU_OPT_SGD) {
    MAU_REQUIRE(weight_decay >= 0.f && (!nesterov || beta1 > 0.f), "opt_pack_step: SGD needs weight_decay >= 0 and, for nesterov, a momentum");
  } else {
    MAU_REQUIRE(step && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "opt_pack_step: Adam needs a device step count and betas in [0, 1)");
  }
  const size_t lds = (size_t)64 * OPT_ROW * sizeof(float);
  const hipStream_t st = (hipStream_t)stream;
  const AdamWPackDesc* tb = (const AdamWPackDesc*)descs;
#define MAU_OPT_LAUNCH(R)                                                                                                      \
  MAU_DISPATCH_DTYPE(dtype, {                                                                                                  \
    MAU_LDS_ATTR(lds, &opt_pack_kernel<T, R>);                                                                                 \
    MAU_LAUNCH((opt_pack_kernel<T, R>), dim3(total_tiles), dim3(1024), lds, st, tb, n, step, grad_scale, lr, beta1, beta2, eps, \
               weight_decay, nesterov);                                                                                       \
  })
  if (rule == MAU_OPT_ADAMW) MAU_OPT_LAUNCH(MAU_OPT_ADAMW);
  else if (rule == MAU_OPT_ADAM) MAU_OPT_LAUNCH(MAU_OPT_ADAM);
  else MAU_OPT_LAUNCH(MAU_OPT_SGD);
#undef MAU_OPT_LAUNCH
  return check_launch("opt_pack_kernel");
}

int mau_grad_norm_chunk(void) { return NORM_CHUNK; }
size_t mau_grad_norm_seg_bytes(void) { return sizeof(NormSeg); }

int mau_grad_norm_seg_fill(void* segs_host, int index, const float* ptr, int64_t n, int block0, int* next_block_host) {
  MAU_REQUIRE(segs_host && next_block_host && index >= 0 && ptr && n > 0 && block0 >= 0 && ((uintptr_t)ptr & 3) == 0,
              "grad_norm_seg_fill: bad arguments");
  const int64_t nb = (n + NORM_CHUNK - 1) / NORM_CHUNK;
  MAU_REQUIRE(block0 + nb < (int64_t)1 << 30, "grad_norm_seg_fill: too many blocks");
  NormSeg* s = reinterpret_cast<NormSeg*>(segs_host) + index;
  s->ptr = ptr; s->n = n; s->block0 = block0; s->pad = 0;
  *next_block_host = block0 + (int)nb;
  return MAU_OK;
}

int mau_grad_norm_clip(const void* segs, int nsegs, int total_blocks, double* ws, unsigned* tickets, float max_norm, float* norm_out,
                       float* coef_out, mau_stream_t stream) {
  MAU_REQUIRE(segs && ws && tickets && norm_out && coef_out && nsegs > 0 && total_blocks >= nsegs && max_norm > 0.f,
              "grad_norm_clip: bad arguments");
  MAU_LAUNCH(grad_norm_clip_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, (const NormSeg*)segs, nsegs, ws, tickets, max_norm,
             norm_out, coef_out);
  return check_launch("grad_norm_clip_kernel");
}

}  // extern "C"
