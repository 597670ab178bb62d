// Text-tower, loss, optimiser and small plumbing kernels.  All HBM / latency bound.
//   embedding gather  tf.nn.embedding_lookup            image_text_model/im_text_rnn_model.py:85
//   LSTM cell         BasicLSTMCell + dynamic_rnn mask  im_text_rnn_model.py:89-90 (A7/A8)
//   softmax CE        slim.losses.softmax_cross_entropy im_text_rnn_model.py:124-125 (A9)
//   Adam              tf.train.AdamOptimizer            im_text_rnn_model.py:134-135 (A10)
#include <stdlib.h>
#include "ds_common.h"

namespace {

// ---- embedding gather: one wavefront per row, rows written in the LSTM's time-major order ----------
// A wave owns RPW consecutive (b, t) positions.  Per position: the id is a wave-uniform scalar load, the row is
// VEC-wide vectors handed to lanes 0, 1, ... (D = 300 -> 75 float4: one full and one 11-lane instruction), no
// per-element integer division.  Four rows are fetched before the first is stored (memory-level parallelism:
// the 12 MB table is cache resident, the stores are the HBM stream) and the stores are non-temporal -- the
// rows are next read by the projection GEMM, long after they left the caches at 2^20 tokens.
template <int VEC, bool OUTORDER = false>
__global__ __launch_bounds__(256) void gather_rows_kernel(const float *table, const int64_t *ids, float *out, int B,
                                                          int T, int D, int64_t rows, int time_major, int rpw) {
    typedef float vec_t __attribute__((ext_vector_type(VEC)));
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t total = (int64_t)B * T;
    int64_t r = wave * rpw;
    const int64_t r1 = r + rpw < total ? r + rpw : total;
    if (r >= r1) return;
    const int DV = D / VEC;
    // OUTORDER (time-major output): r walks the OUTPUT rows t * B + b, so a wave's stores -- and the stores of
    // consecutive waves -- form one linear stream (the ids are then read with stride T: 8 MB of scattered 8-byte reads
    // against 1.26 GB of row stores); otherwise r walks the id list and a time-major row lands B * D floats from the next
    int b, t;
    if (OUTORDER) { t = (int)(r / B); b = (int)(r - (int64_t)t * B); }
    else { b = (int)(r / T); t = (int)(r - (int64_t)b * T); }     // once per wave; then incremented
    constexpr int U = 4;                                           // rows in flight
    if (VEC == 4 && DV <= 128) {
        // Rows of at most 128 float4 (two chunks per lane), software pipelined: the id reads and the eight row loads of
        // the NEXT four rows go out before the stores of the current four.  In the plain loop below every load sits
        // behind the previous chunk's stores and waits for them (one in-order memory counter): two round trips per group.
        const float *srcA[U], *srcB[U];
        float *dstA[U], *dstB[U];
        bool okA[U], okB[U];
        vec_t a0[U], a1[U], b0[U], b1[U];
        auto fetch = [&](int64_t rr, const float *(&src)[U], float *(&dst)[U], bool (&ok)[U], vec_t (&v0)[U], vec_t (&v1)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = rr + u < r1;
                const int64_t id = in ? ids[OUTORDER ? (int64_t)b * T + t : rr + u] : -1;               // wave-uniform
                ok[u] = id >= 0 && id < rows;                          // out-of-range id -> zero row
                src[u] = table + (ok[u] ? id : 0) * D;
                dst[u] = in ? out + (OUTORDER ? rr + u : (time_major ? (int64_t)t * B + b : rr + u)) * D : nullptr;
                if (OUTORDER) { if (++b == B) { b = 0; ++t; } }
                else if (++t == T) { t = 0; ++b; }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                v0[u] = vec_t(0.f);
                v1[u] = vec_t(0.f);
                if (lane < DV && ok[u]) v0[u] = *reinterpret_cast<const vec_t *>(src[u] + lane * VEC);
                if (64 + lane < DV && ok[u]) v1[u] = *reinterpret_cast<const vec_t *>(src[u] + (64 + lane) * VEC);
            }
        };
        auto put = [&](float *(&dst)[U], vec_t (&v0)[U], vec_t (&v1)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!dst[u]) continue;
                if (lane < DV) __builtin_nontemporal_store(v0[u], reinterpret_cast<vec_t *>(dst[u] + lane * VEC));
                if (64 + lane < DV) __builtin_nontemporal_store(v1[u], reinterpret_cast<vec_t *>(dst[u] + (64 + lane) * VEC));
            }
        };
        fetch(r, srcA, dstA, okA, a0, a1);
        for (; r < r1; r += 2 * U) {
            if (r + U < r1) fetch(r + U, srcB, dstB, okB, b0, b1);
            put(dstA, a0, a1);
            if (r + U >= r1) break;
            if (r + 2 * U < r1) fetch(r + 2 * U, srcA, dstA, okA, a0, a1);
            put(dstB, b0, b1);
        }
        return;
    }
    for (; r < r1; r += U) {
        const float *src[U];
        float *dst[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = r + u < r1;
            const int64_t id = in ? ids[OUTORDER ? (int64_t)b * T + t : r + u] : -1;               // wave-uniform
            ok[u] = id >= 0 && id < rows;                          // out-of-range id -> zero row
            src[u] = table + (ok[u] ? id : 0) * D;
            dst[u] = in ? out + (OUTORDER ? r + u : (time_major ? (int64_t)t * B + b : r + u)) * D : nullptr;
            if (OUTORDER) { if (++b == B) { b = 0; ++t; } }
            else if (++t == T) { t = 0; ++b; }
        }
        for (int v0 = 0; v0 < DV; v0 += 64) {
            const int v = v0 + lane;
            vec_t val[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                val[u] = vec_t(0.f);
                if (v < DV && ok[u]) val[u] = *reinterpret_cast<const vec_t *>(src[u] + v * VEC);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (v < DV && dst[u]) __builtin_nontemporal_store(val[u], reinterpret_cast<vec_t *>(dst[u] + v * VEC));
        }
    }
}

// ---- embedding gradient: deterministic wavefront-reduced scatter-add ------------------------------
// dtable[v, :] = sum over the positions p = b*T + t with ids[p] == v of dx[row(p), :], one wave per
// vocabulary row.  The wave sweeps the id list 64 positions at a time, ballots the matches and adds the
// matching rows in ascending position order -- no atomics, no sort, bit-reproducible -- with lane l owning
// columns l, l+64, ... of the row.  Rows nobody referenced come out as zeros (the whole table is written).
// Not reachable from the reference graph (its embedding is trainable=False, im_text_rnn_model.py:82); it
// backs the optional full fine-tuning switch.
template <int NQ>
__global__ __launch_bounds__(256) void embedding_grad_kernel(const float *dx, const int64_t *ids, float *dtable, int B,
                                                             int T, int D, int64_t rows, int time_major) {
    const int lane = threadIdx.x & 63;
    const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= rows) return;
    float acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
    const int BT = B * T;
    for (int base = 0; base < BT; base += 64) {
        const int pos = base + lane;
        const int64_t id = pos < BT ? ids[pos] : -1;
        unsigned long long mask = __ballot(id == v);
        while (mask) {
            const int j = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const int p = base + j;
            const int b = p / T, t = p - b * T;
            const float *src = dx + (time_major ? (int64_t)t * B + b : (int64_t)p) * D;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int c = lane + 64 * q;
                if (c < D) acc[q] += src[c];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int c = lane + 64 * q;
        if (c < D) dtable[v * D + c] = acc[q];
    }
}

// ---- LSTM cell -----------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }

__global__ __launch_bounds__(256) void lstm_cell_fwd_kernel(float *gates, const float *rec, int nslabs,
                                                            int64_t slab_stride, const float *c_prev,
                                                            const float *h_prev, const int64_t *seq_len, int t, int B,
                                                            int H, float forget_bias, float *c_out, float *h_out) {
    const int64_t total = (int64_t)B * H;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int b = (int)(i / H), h = (int)(i - (int64_t)b * H);
        float *g = gates + (int64_t)b * 4 * H + h;
        float pi = g[0], pj = g[H], pf = g[2 * H], po = g[3 * H];     // x_t*Wx + bias (hoisted GEMM)
        for (int s = 0; s < nslabs; ++s) {                             // + h_{t-1}*Wh, split-K slabs
            const float *r = rec + s * slab_stride + (int64_t)b * 4 * H + h;
            pi += r[0]; pj += r[H]; pf += r[2 * H]; po += r[3 * H];
        }
        const float si = sigmoidf_(pi);
        const float tj = tanhf(pj);
        const float sf = sigmoidf_(pf + forget_bias);
        const float so = sigmoidf_(po);
        const float cp = c_prev[i], hp = h_prev[i];
        const float cn = cp * sf + si * tj;
        const float hn = tanhf(cn) * so;
        const bool live = (int64_t)t < seq_len[b];
        g[0] = si;
        g[H] = tj;
        g[2 * H] = sf;
        g[3 * H] = so;
        c_out[i] = live ? cn : cp;      // dynamic_rnn copies the state through past seq_len
        h_out[i] = live ? hn : hp;
    }
}

__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(const float *acts, const float *c_t, const float *c_prev,
                                                            const float *dh, const float *dh_slabs, int nslabs,
                                                            int64_t slab_stride, const float *dc,
                                                            const int64_t *seq_len, int t, int B, int H,
                                                            float *dgates, float *dc_prev, float *dh_carry) {
    const int64_t total = (int64_t)B * H;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int b = (int)(i / H), h = (int)(i - (int64_t)b * H);
        const float *a = acts + (int64_t)b * 4 * H + h;
        float *dg = dgates + (int64_t)b * 4 * H + h;
        const bool live = (int64_t)t < seq_len[b];
        float dhv = dh[i];                                     // carried / injected part of d(loss)/d(h_t)
        for (int s = 0; s < nslabs; ++s) dhv += dh_slabs[s * slab_stride + i];   // + dgates_{t+1}*Wh^T (split-K slabs)
        const float dcv = dc[i];
        if (live) {
            const float si = a[0], tj = a[H], sf = a[2 * H], so = a[3 * H];
            const float tc = tanhf(c_t[i]);
            const float dct = dcv + dhv * so * (1.f - tc * tc);
            dg[0] = dct * tj * si * (1.f - si);
            dg[H] = dct * si * (1.f - tj * tj);
            dg[2 * H] = dct * c_prev[i] * sf * (1.f - sf);
            dg[3 * H] = dhv * tc * so * (1.f - so);
            dc_prev[i] = dct * sf;
            dh_carry[i] = 0.f;
        } else {
            dg[0] = 0.f;
            dg[H] = 0.f;
            dg[2 * H] = 0.f;
            dg[3 * H] = 0.f;
            dc_prev[i] = dcv;
            dh_carry[i] = dhv;
        }
    }
}

// ---- softmax cross entropy (+ gradient), one workgroup, fixed summation order -----------------------
// (the whole workgroup's work: softmax_ce_kernel, and slab_epilogue_ce_kernel behind its combine -- there thread t reads back
// the rows t, t + 256 of `logits` that it has just stored itself)
// OPTS = false is slim.losses.softmax_cross_entropy at its defaults, the text the two entry points have always run.
// OPTS = true adds its two other arguments (ds_ce_desc): label_smoothing eps -- q = onehot (1 - eps) + eps / C, TF's own
// form -- and per-class weights w_b = cw[y_b] under compute_weighted_loss's SUM_BY_NONZERO_WEIGHTS: loss = sum_b w_b l_b / P,
// l_b = sum_c q_bc (lse_b - z_bc), dlogits = (softmax - q) w_b grad_scale / P, P = #{b: w_b != 0} counted by a first pass over
// the labels (integers: exact in any order; reduced in the fixed order of the loss all the same).  P == 0: loss and dlogits
// are 0.  With eps = 0 and w = 1 every product below is by 1 or 0 and P = B: the bits of OPTS = false (finite logits).
template <bool OPTS>
__device__ __forceinline__ void softmax_ce_workgroup(const float *logits, const int64_t *labels, int B, int C,
                                                     float grad_scale, const float *grad_scale_dev,
                                                     float *loss, float *dlogits, float *red, float eps = 0.f,
                                                     const float *cw = nullptr) {
    if (grad_scale_dev) grad_scale *= grad_scale_dev[0];   // upstream d(loss) handed over on device
    float denom = (float)B, sp = 1.f, sn = 0.f;
    if constexpr (OPTS) {
        int *cnt = reinterpret_cast<int *>(red);
        int n = 0;
        for (int b = threadIdx.x; b < B; b += 256) {
            const int64_t yl = labels[b];
            // (the lookup is guarded exactly as the row pass guards it: a label outside [0, C) weighs 1)
            const float w = (cw && yl >= 0 && yl < C) ? cw[yl] : 1.f;
            n += w != 0.f ? 1 : 0;
        }
        cnt[threadIdx.x] = n;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (threadIdx.x < o) cnt[threadIdx.x] += cnt[threadIdx.x + o];
            __syncthreads();
        }
        denom = (float)cnt[0];
        __syncthreads();                                   // `red` is the loss reduction's next
        sp = 1.f - eps;
        sn = eps / (float)C;
    }
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float *z = logits + (int64_t)b * C;
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) m = fmaxf(m, z[c]);
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += expf(z[c] - m);
        // a label outside [0, C) (dataset converted for another class list) must not index out of bounds:
        // it poisons the loss with NaN so the run stops visibly; one_hot() of such a label is all zeros in TF
        const int64_t yl = labels[b];
        const bool yok = yl >= 0 && yl < C;
        const int y = yok ? (int)yl : -1;
        if constexpr (OPTS) {
            const float w = (cw && yok) ? cw[y] : 1.f;
            if (w != 0.f) {                                // (a zero weight drops the row, whatever its logits)
                const float lse = m + logf(s);
                float l = 0.f;
                for (int c = 0; c < C; ++c) l += ((c == y ? sp : 0.f) + sn) * (lse - z[c]);
                acc += yok ? w * l : NAN;
            }
            if (dlogits) {
                const float wk = denom > 0.f ? w * (grad_scale / denom) : 0.f, inv = 1.f / s;
                for (int c = 0; c < C; ++c)
                    dlogits[(int64_t)b * C + c] =
                        wk == 0.f ? 0.f : (expf(z[c] - m) * inv - ((c == y ? sp : 0.f) + sn)) * wk;
            }
        } else {
            acc += yok ? (m + logf(s)) - z[y] : NAN;
            if (dlogits) {
                const float k = grad_scale / (float)B, inv = 1.f / s;
                for (int c = 0; c < C; ++c)
                    dlogits[(int64_t)b * C + c] = (expf(z[c] - m) * inv - (c == y ? 1.f : 0.f)) * k;
            }
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if constexpr (OPTS) {
        if (threadIdx.x == 0 && loss) loss[0] = denom > 0.f ? red[0] / denom : 0.f;
    } else {
        if (threadIdx.x == 0 && loss) loss[0] = red[0] / (float)B;
    }
}

template <bool OPTS>
__global__ __launch_bounds__(256) void softmax_ce_kernel(const float *logits, const int64_t *labels, int B, int C,
                                                         float grad_scale, const float *grad_scale_dev,
                                                         float *loss, float *dlogits, float eps, const float *cw) {
    __shared__ float red[256];
    softmax_ce_workgroup<OPTS>(logits, labels, B, C, grad_scale, grad_scale_dev, loss, dlogits, red, eps, cw);
}

// ---- TF Adam over a flat buffer ------------------------------------------------------------------
// What compute_gradients(total_loss) returns for element i (w = theta[i]): the (all-reduced, clone-summed) gradient times
// grad_scale plus the L2 regulariser's term on the first n_wd entries.  ONE definition: ds_adam_tf, ds_adam_tf_clipped and the
// norm pass of ds_grad_norms evaluate it.  No contraction into fused multiply-adds, here and in adam_tf_update: the
// compiler forms them in one caller's loop and not in another's (it did, in an unrolled norm loop), and the three kernels
// must round alike -- products and sums, each rounded once, which is what adam_tf_kernel has always compiled to.
__device__ __forceinline__ float adam_g_eff(const float *g, int64_t i, float w, int64_t n_wd, float wd, float grad_scale) {
#pragma clang fp contract(off)
    float gi = g[i] * grad_scale;
    if (i < n_wd) gi += wd * w;                       // d/dw of wd * sum(w^2)/2
    return gi;
}

// The update of element i from its effective gradient gi, shared by every Adam kernel; returns the new theta[i].
__device__ __forceinline__ float adam_tf_update(float *theta, float *m, float *v, int64_t i, float w, float gi, float lr_t,
                                                float b1, float b2, float eps) {
#pragma clang fp contract(off)
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float wn = w - lr_t * mi / (sqrtf(vi) + eps);     // epsilon outside the bias correction (A10)
    theta[i] = wn;
    return wn;
}

// ---- the other optimisers of slim's --optimizer behind the same effective gradient (ds_opt_step) ---------------------------
// [TF-sem] TF's training_ops CPU functors restated (TensorFlow is not in the reference tree; parity unpinned).  Every
// operation below is one fp32 rounding, in this order; nothing is contracted.  slot0 / slot1 are the buffers Adam calls m / v.
enum { kOptAdam = DS_OPT_ADAM, kOptSgd = DS_OPT_SGD, kOptMomentum = DS_OPT_MOMENTUM, kOptRmsprop = DS_OPT_RMSPROP };

// ApplyGradientDescent: no slot is read or written.
__device__ __forceinline__ float sgd_tf_update(float *theta, int64_t i, float w, float gi, float lr) {
#pragma clang fp contract(off)
    const float p = lr * gi;
    const float wn = w - p;
    theta[i] = wn;
    return wn;
}

// ApplyMomentum, use_nesterov = False: acc (slot0, starts at 0) = mu * acc + g; theta -= lr * acc.
__device__ __forceinline__ float momentum_tf_update(float *theta, float *acc, int64_t i, float w, float gi, float lr, float mu) {
#pragma clang fp contract(off)
    const float t = mu * acc[i];
    const float a = t + gi;
    acc[i] = a;
    const float p = lr * a;
    const float wn = w - p;
    theta[i] = wn;
    return wn;
}

// ApplyRMSProp: ms (slot1, starts at 1) += (g^2 - ms) (1 - rho); mom (slot0, starts at 0) = mom * mu + g lr / sqrt(ms + eps);
// theta -= mom.
__device__ __forceinline__ float rmsprop_tf_update(float *theta, float *mom, float *ms, int64_t i, float w, float gi, float lr,
                                                   float mu, float rho, float eps) {
#pragma clang fp contract(off)
    const float q = gi * gi;
    const float msi = ms[i];
    const float d = q - msi;
    const float e = d * (1.f - rho);
    const float msn = msi + e;
    ms[i] = msn;
    const float s = sqrtf(msn + eps);
    const float nmr = gi * lr;
    const float r = nmr / s;
    const float t = mom[i] * mu;
    const float mn = t + r;
    mom[i] = mn;
    const float wn = w - mn;
    theta[i] = wn;
    return wn;
}

// The update of kind KIND on element i; lr is Adam's lr_t for kOptAdam, the learning rate otherwise.  Returns the new theta[i].
template <int KIND>
__device__ __forceinline__ float opt_update(float *theta, float *slot0, float *slot1, int64_t i, float w, float gi, float lr,
                                            float b1, float b2, float eps, float mu, float rho) {
    if (KIND == kOptSgd) return sgd_tf_update(theta, i, w, gi, lr);
    if (KIND == kOptMomentum) return momentum_tf_update(theta, slot0, i, w, gi, lr, mu);
    if (KIND == kOptRmsprop) return rmsprop_tf_update(theta, slot0, slot1, i, w, gi, lr, mu, rho, eps);
    return adam_tf_update(theta, slot0, slot1, i, w, gi, lr, b1, b2, eps);
}

// tf.train.ExponentialMovingAverage's assign_moving_average on element i, wn = the variable after the update:
// shadow -= (shadow - wn) * rate -- a difference, a product and a difference, each rounded once (the _ema kernels).
__device__ __forceinline__ void ema_update(float *shadow, int64_t i, float wn, float rate) {
#pragma clang fp contract(off)
    const float s = shadow[i];
    const float d = s - wn;
    const float p = d * rate;
    shadow[i] = s - p;
}

// The unclipped loop shape of every optimiser kind.  KIND = kOptAdam, EMA = false: ds_adam_tf (shadow, ema_rate and
// ema_rate_dev are not read).  EMA = true: ds_adam_tf_ema, the same pass with the shadow update behind every element's update.
// The other kinds (ds_opt_step) read lr_t as the learning rate and m / v as slot0 / slot1.
template <int KIND, bool EMA>
__global__ __launch_bounds__(256) void adam_tf_kernel(float *theta, const float *g, float *m, float *v, float *shadow,
                                                      int64_t n, int64_t n_wd, float wd, float grad_scale, float lr_t,
                                                      const float *lr_t_dev, float ema_rate, const float *ema_rate_dev,
                                                      float b1, float b2, float eps, float mu, float rho) {
    if (lr_t_dev) lr_t = lr_t_dev[0];         // step size kept on device (hipGraph replay safe)
    if (EMA && ema_rate_dev) ema_rate = ema_rate_dev[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float w = theta[i];
        const float wn = opt_update<KIND>(theta, m, v, i, w, adam_g_eff(g, i, w, n_wd, wd, grad_scale), lr_t, b1, b2, eps, mu,
                                          rho);
        if (EMA) ema_update(shadow, i, wn, ema_rate);
    }
}

// ---- gradient norms, clipping factors and the non-finite guard (ds_grad_norms, ds_adam_tf_clipped) -------------------------
// Tables (int64, built by the host once per parameter layout):
//   segment s = one TF variable: {offset, rows, ld, c0, ncols, chunk0, nchunks, 0} -- element k of it (k < rows * ncols) is
//               flat element offset + (k / ncols) * ld + c0 + k % ncols (a plain variable: rows = 1, ld = ncols, c0 = 0; a
//               column range of a horizontally fused tensor otherwise); its chunks are chunk0 .. chunk0 + nchunks - 1
//   chunk c   = {seg, k0, count, 0}: elements k0 .. k0 + count - 1 of segment seg; seg = -1: `count` pad elements from flat
//               element k0 on (they belong to no variable; the optimiser visits them with factor 1)
// A chunk never straddles a segment, so a workgroup's sum belongs to one variable and the optimiser reads ONE factor per
// workgroup.  Every chunk's flat range is checked against n before it is walked (a chunk that fails is left out as a whole): a
// broken table cannot make a kernel leave the buffers.
constexpr int kSegWords = 8, kChunkWords = 4;
enum { kFlagNonfinite = 0, kFlagSkip = 1, kFlagSkipped = 2 };

struct ClipChunk {
    int64_t seg, k0, count, offset, ld, c0, ncols;
    bool plain, ok;
};

__device__ __forceinline__ ClipChunk clip_chunk(const int64_t *segments, int nseg, const int64_t *chunks, int c, int64_t n) {
    ClipChunk q;
    q.seg = chunks[(int64_t)c * kChunkWords];
    q.k0 = chunks[(int64_t)c * kChunkWords + 1];
    q.count = chunks[(int64_t)c * kChunkWords + 2];
    q.ok = q.seg >= -1 && q.seg < nseg && q.k0 >= 0 && q.count >= 0 && q.count <= n;
    if (q.seg < 0 || !q.ok) {          // pad elements: flat from k0
        q.offset = 0; q.ld = 1; q.c0 = 0; q.ncols = 1; q.plain = true;
        q.ok = q.ok && q.k0 <= n - q.count;
        return q;
    }
    const int64_t *s = segments + q.seg * kSegWords;
    const int64_t rows = s[1];
    q.offset = s[0]; q.ld = s[2]; q.c0 = s[3]; q.ncols = s[4];
    q.plain = q.ld == q.ncols;
    // the segment lies inside [0, n) (its last element is offset + (rows - 1) ld + c0 + ncols - 1) and the chunk inside the segment
    q.ok = q.offset >= 0 && q.offset < n && rows > 0 && rows <= n && q.ncols > 0 && q.ld >= q.ncols && q.ld <= n && q.c0 >= 0 &&
           q.c0 + q.ncols <= q.ld && q.c0 + q.ncols <= n - q.offset && rows - 1 <= (n - q.offset - q.c0 - q.ncols) / q.ld &&
           q.k0 <= rows * q.ncols - q.count;
    return q;
}

// flat index of element j (j < count) of a chunk that clip_chunk found inside the buffers
__device__ __forceinline__ int64_t clip_flat(const ClipChunk &q, int64_t j) {
    const int64_t k = q.k0 + j;
    if (q.plain) return q.offset + q.c0 + k;
    const int64_t r = (k | q.ncols) >> 32 ? k / q.ncols : (int64_t)((uint32_t)k / (uint32_t)q.ncols);
    return q.offset + r * q.ld + q.c0 + (k - r * q.ncols);
}

// sum over the workgroup, in double, in a fixed order: thread t's own terms in index order, then the tree below
__device__ __forceinline__ double block_sum_f64(double acc, double *red) {
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// Stage 1: partials[c] = sum of g_eff^2 over chunk c (0 for a pad chunk).  g_eff in fp32 as the optimiser forms it, the
// squares and the sums in double.  The chunks are walked grid-stride, so the result does not depend on the grid.
__global__ __launch_bounds__(256) void grad_norms_stage1(const float *theta, const float *g, int64_t n, int64_t n_wd, float wd,
                                                         float grad_scale, const int64_t *segments, int nseg,
                                                         const int64_t *chunks, int nchunks, double *partials) {
    __shared__ double red[256];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const ClipChunk q = clip_chunk(segments, nseg, chunks, c, n);
        double acc = 0.0;
        if (q.ok && q.seg >= 0) {
#pragma unroll 4
            for (int64_t j = threadIdx.x; j < q.count; j += 256) {
                const int64_t i = clip_flat(q, j);
                const double ge = (double)adam_g_eff(g, i, theta[i], n_wd, wd, grad_scale);
                acc += ge * ge;
            }
        }
        const double s = block_sum_f64(acc, red);
        if (threadIdx.x == 0) partials[c] = s;
    }
}

__device__ __forceinline__ float clip_factor(double sumsq, double clip) {
    if (!(fabs(sumsq) <= 1.7976931348623157e308)) return __builtin_nanf("");      // NaN or Inf norm: fmax would drop the NaN
    const double nrm = sqrt(sumsq);
    return (float)(clip / (nrm > clip ? nrm : clip));                             // exactly 1.0f when nothing clips
}

// Stage 2, one workgroup: sumsq[s] = the partials of segment s added in chunk order, sumsq[nseg] = the segment sums added in
// segment order; flags[0] = some sum is NaN / Inf, flags[1] = the step is to be skipped (that, under the guard);
// factors[s] = what the optimiser multiplies segment s by, factors[nseg] = the global factor (1 unless mode 2).
// mode 0: no clipping, 1: tf.clip_by_norm per variable, 2: tf.clip_by_global_norm.
__global__ __launch_bounds__(256) void grad_norms_stage2(const int64_t *segments, int nseg, int nchunks, const double *partials,
                                                         int mode, double clip, int guard, double *sumsq, float *factors,
                                                         int *flags) {
    __shared__ int bad;
    __shared__ float gfac;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    for (int s = threadIdx.x; s < nseg; s += 256) {
        int64_t c0 = segments[(int64_t)s * kSegWords + 5], c1 = c0 + segments[(int64_t)s * kSegWords + 6];
        if (c0 < 0) c0 = 0;
        if (c1 > nchunks) c1 = nchunks;
        double acc = 0.0;
        int64_t c = c0;
        for (; c + 8 <= c1; c += 8) {          // eight loads in flight, added in chunk order
            double p[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) p[j] = partials[c + j];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += p[j];
        }
        for (; c < c1; ++c) acc += partials[c];
        sumsq[s] = acc;
        if (!(fabs(acc) <= 1.7976931348623157e308)) bad = 1;      // (every writer stores the same value)
        if (mode != 2) factors[s] = mode == 1 ? clip_factor(acc, clip) : 1.f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int s = 0; s < nseg; ++s) tot += sumsq[s];
        sumsq[nseg] = tot;
        if (!(fabs(tot) <= 1.7976931348623157e308)) bad = 1;
        gfac = mode == 2 ? clip_factor(tot, clip) : 1.f;
        factors[nseg] = gfac;
        flags[kFlagNonfinite] = bad;
        flags[kFlagSkip] = bad && guard ? 1 : 0;
    }
    __syncthreads();
    if (mode == 2)
        for (int s = threadIdx.x; s < nseg; s += 256) factors[s] = gfac;
}

// The optimiser launch behind ds_grad_norms, the clipped loop shape of every kind: chunk by chunk, g_eff * factors[seg] into
// the per-element update.  flags[1] set: nothing is written but flags[2], the count of skipped steps, which workgroup 0 raises
// by one.  EMA = true (ds_adam_tf_clipped_ema): the shadow update behind every element's update, pad elements included; a
// skipped step leaves the shadows alone too.
template <int KIND, bool EMA>
__global__ __launch_bounds__(256) void adam_tf_clipped_kernel(float *theta, const float *g, float *m, float *v, float *shadow,
                                                              int64_t n, int64_t n_wd, float wd, float grad_scale, float lr_t,
                                                              const float *lr_t_dev, float ema_rate,
                                                              const float *ema_rate_dev, float b1, float b2, float eps,
                                                              float mu, float rho, const int64_t *segments, int nseg,
                                                              const int64_t *chunks, int nchunks, const float *factors,
                                                              int *flags) {
    if (flags[kFlagSkip]) {
        if (blockIdx.x == 0 && threadIdx.x == 0) flags[kFlagSkipped] = flags[kFlagSkipped] + 1;
        return;
    }
    if (lr_t_dev) lr_t = lr_t_dev[0];
    if (EMA && ema_rate_dev) ema_rate = ema_rate_dev[0];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const ClipChunk q = clip_chunk(segments, nseg, chunks, c, n);
        if (!q.ok) continue;
        const float f = q.seg >= 0 ? factors[q.seg] : 1.f;
#pragma unroll 4
        for (int64_t j = threadIdx.x; j < q.count; j += 256) {
            const int64_t i = clip_flat(q, j);
            const float w = theta[i];
            const float wn = opt_update<KIND>(theta, m, v, i, w, adam_g_eff(g, i, w, n_wd, wd, grad_scale) * f, lr_t, b1, b2,
                                              eps, mu, rho);
            if (EMA) ema_update(shadow, i, wn, ema_rate);
        }
    }
}

// ---- clone-gradient accumulation over the flat gradient buffer -----------------------------------------
// One float4 per thread and trip: element i is read and written by the same thread only, so acc and g may be any two
// buffers (or the same one) and the result does not depend on the launch shape.  The running sum is the LEFT operand of a
// plain fp32 add (no contraction is possible: there is no multiply).  Plain loads and stores: the sum is read next by the
// all-reduce / Adam, the running sum by the next clone -- both want it in L2 / the Infinity Cache.
constexpr int kAccumVecPerBlock = 256 * 4;       // four 16-byte trips per thread before the grid cap takes over

template <int MODE>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float4 *acc, float4 *g, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 b = g[i];
        if (MODE == 0) {
            acc[i] = b;
        } else {
            const float4 a = acc[i];
            const float4 s = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
            if (MODE == 1) acc[i] = s;
            else g[i] = s;
        }
    }
}

// ---- reductions / plumbing ---------------------------------------------------------------------------
constexpr int kSumsqBlocks = 256;

__global__ __launch_bounds__(256) void sumsq_stage1(const float *x, int64_t n, float *partials) {
    __shared__ float red[256];
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) acc += x[i] * x[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void sum_stage2(const float *partials, int n, float *out) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += (double)partials[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)red[0];
}

// column sums of x[M, C] (BiasAddGrad): grid (C/64, RS); thread = (column, one of 4 row lanes)
__global__ __launch_bounds__(256) void colsum_stage1(const float *x, int64_t M, int C, int ld, int rows_per_split,
                                                     float *partials) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_split;
    int64_t r1 = r0 + rows_per_split;
    if (r1 > M) r1 = M;
    float acc = 0.f;
    if (c < C)
        for (int64_t r = r0 + rl; r < r1; r += 4) acc += x[r * ld + c];
    red[rl][cl] = acc;
    __syncthreads();
    if (rl == 0 && c < C) partials[(int64_t)blockIdx.y * C + c] = red[0][cl] + red[1][cl] + red[2][cl] + red[3][cl];
}

// few row splits (M <= 512: the head biases at B <= 512): both stages in one launch, split by split in the same
// arithmetic and order (fp32 over 4 row lanes per split, double over the splits) -- same bits, one dispatch less
__global__ __launch_bounds__(256) void colsum_small_kernel(const float *x, int64_t M, int C, int ld, int rows_per_split,
                                                           int RS, float *out) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    double total = 0.0;
    for (int s = 0; s < RS; ++s) {
        const int64_t r0 = (int64_t)s * rows_per_split;
        int64_t r1 = r0 + rows_per_split;
        if (r1 > M) r1 = M;
        float acc = 0.f;
        if (c < C)
            for (int64_t r = r0 + rl; r < r1; r += 4) acc += x[r * ld + c];
        __syncthreads();
        red[rl][cl] = acc;
        __syncthreads();
        if (rl == 0) total += (double)(red[0][cl] + red[1][cl] + red[2][cl] + red[3][cl]);
    }
    if (rl == 0 && c < C) out[c] = (float)total;
}

__global__ __launch_bounds__(256) void colsum_stage2(const float *partials, int RS, int C, float *out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double acc = 0.0;
    for (int s = 0; s < RS; ++s) acc += (double)partials[(int64_t)s * C + c];
    out[c] = (float)acc;
}

__global__ __launch_bounds__(256) void copy2d_kernel(const float *src, int lds, float *dst, int ldd, int64_t rows,
                                                     int cols) {
    const int64_t total = rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cols;
        const int c = (int)(i - r * cols);
        dst[r * ldd + c] = src[r * lds + c];
    }
}

__global__ __launch_bounds__(256) void pad_channels_kernel(const float *src, int cs, float *dst, int cd,
                                                           int64_t pixels) {
    const int64_t total = pixels * cd;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t p = i / cd;
        const int c = (int)(i - p * cd);
        dst[i] = c < cs ? src[p * cs + c] : 0.f;
    }
}

__global__ __launch_bounds__(256) void fill_kernel(float *dst, int64_t n, float value) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = value;
}

// ds_token_dot: out[b, t] = sum_d dx[t*B + b, d] * x[t*B + b, d] (gradient x input per word) over the text tower's time-major
// buffers.  One wave per row: 16-byte loads where D and the addresses allow, fp32 products added per lane in index order,
// then the wave's butterfly -- a fixed order, so repeated runs give the same bits.  Rows past the post's length write 0
// without reading.
template <int VEC>
__global__ __launch_bounds__(256) void token_dot_kernel(const float *dx, const float *x, const int64_t *seq_len, float *out,
                                                        int B, int T, int D) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // t * B + b
    if (row >= (int64_t)T * B) return;                                      // (wave-uniform)
    const int t = (int)(row / B), b = (int)(row - (int64_t)t * B);
    float acc = 0.f;
    if ((int64_t)t < seq_len[b]) {
        const float *a = dx + row * D, *e = x + row * D;
        if (VEC == 4) {
            for (int d = lane * 4; d < D; d += 256) {
                const float4 u = *reinterpret_cast<const float4 *>(a + d), v = *reinterpret_cast<const float4 *>(e + d);
                acc = __builtin_fmaf(u.x, v.x, acc);
                acc = __builtin_fmaf(u.y, v.y, acc);
                acc = __builtin_fmaf(u.z, v.z, acc);
                acc = __builtin_fmaf(u.w, v.w, acc);
            }
        } else {
            for (int d = lane; d < D; d += 64) acc = __builtin_fmaf(a[d], e[d], acc);
        }
        acc = ds::wave_sum(acc);
    }
    if (lane == 0) out[(int64_t)b * T + t] = acc;
}

}  // namespace

extern "C" int ds_gather_rows(const float *table, const int64_t *ids, float *out, int32_t B, int32_t T, int32_t D,
                              int64_t table_rows, int32_t time_major, void *stream) {
    DS_REQUIRE(table && ids && out && B > 0 && T > 0 && D > 0 && table_rows > 0, "ds_gather_rows: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const bool a16 = (((uintptr_t)table | (uintptr_t)out) & 15) == 0, a8 = (((uintptr_t)table | (uintptr_t)out) & 7) == 0;
    const int64_t total = (int64_t)B * T;
    // rows per wave: enough waves to fill the chip several times over, at most 16 rows each
    int rpw = (int)((total + (int64_t)ds::kCUs * 32 * 4 - 1) / ((int64_t)ds::kCUs * 32 * 4));
    rpw = rpw < 4 ? 4 : (rpw > 16 ? 16 : rpw);
    const int64_t waves = (total + rpw - 1) / rpw;
    const dim3 grid((unsigned)((waves + 3) / 4));
    if (D % 4 == 0 && a16 && time_major) {
        hipLaunchKernelGGL((gather_rows_kernel<4, true>), grid, dim3(256), 0, s, table, ids, out, B, T, D, table_rows, time_major, rpw);
    } else if (D % 4 == 0 && a16) {
        hipLaunchKernelGGL(gather_rows_kernel<4>, grid, dim3(256), 0, s, table, ids, out, B, T, D, table_rows, time_major, rpw);
    } else if (D % 2 == 0 && a8) {
        hipLaunchKernelGGL(gather_rows_kernel<2>, grid, dim3(256), 0, s, table, ids, out, B, T, D, table_rows, time_major, rpw);
    } else {
        hipLaunchKernelGGL(gather_rows_kernel<1>, grid, dim3(256), 0, s, table, ids, out, B, T, D, table_rows, time_major, rpw);
    }
    return ds::check_launch("ds_gather_rows");
}

extern "C" int ds_token_dot(const float *dx, const float *x, const int64_t *seq_len, float *out, int32_t B, int32_t T,
                            int32_t D, void *stream) {
    DS_REQUIRE(dx && x && seq_len && out && B > 0 && T > 0 && D > 0, "ds_token_dot: bad argument");
    const int64_t rows = (int64_t)B * T;
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (D % 4 == 0 && ((((uintptr_t)dx) | ((uintptr_t)x)) & 15) == 0)
        hipLaunchKernelGGL(token_dot_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, dx, x, seq_len, out, B, T, D);
    else
        hipLaunchKernelGGL(token_dot_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, dx, x, seq_len, out, B, T, D);
    return ds::check_launch("ds_token_dot");
}

extern "C" int ds_embedding_grad(const float *dx, const int64_t *ids, float *dtable, int32_t B, int32_t T, int32_t D,
                                 int64_t table_rows, int32_t time_major, void *stream) {
    DS_REQUIRE(dx && ids && dtable && B > 0 && T > 0 && D > 0 && D <= 512 && table_rows > 0,
               "ds_embedding_grad: bad argument (D <= 512)");
    const dim3 grid((unsigned)((table_rows + 3) / 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (D <= 64) hipLaunchKernelGGL(embedding_grad_kernel<1>, grid, block, 0, s, dx, ids, dtable, B, T, D, table_rows, time_major);
    else if (D <= 128) hipLaunchKernelGGL(embedding_grad_kernel<2>, grid, block, 0, s, dx, ids, dtable, B, T, D, table_rows, time_major);
    else if (D <= 320) hipLaunchKernelGGL(embedding_grad_kernel<5>, grid, block, 0, s, dx, ids, dtable, B, T, D, table_rows, time_major);
    else hipLaunchKernelGGL(embedding_grad_kernel<8>, grid, block, 0, s, dx, ids, dtable, B, T, D, table_rows, time_major);
    return ds::check_launch("ds_embedding_grad");
}

extern "C" int ds_lstm_cell_fwd(float *gates, const float *rec_slabs, int32_t nslabs, int64_t slab_stride,
                                const float *c_prev, const float *h_prev, const int64_t *seq_len, int32_t t, int32_t B,
                                int32_t H, float forget_bias, float *c_out, float *h_out, void *stream) {
    DS_REQUIRE(gates && c_prev && h_prev && seq_len && c_out && h_out && B > 0 && H > 0 && nslabs >= 0 &&
                   (nslabs == 0 || rec_slabs),
               "ds_lstm_cell_fwd: bad argument");
    hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(ds::stream_grid((int64_t)B * H, 256)), dim3(256), 0,
                       (hipStream_t)stream, gates, rec_slabs, nslabs, slab_stride, c_prev, h_prev, seq_len, t, B, H,
                       forget_bias, c_out, h_out);
    return ds::check_launch("ds_lstm_cell_fwd");
}

extern "C" int ds_lstm_cell_bwd(const float *acts, const float *c_t, const float *c_prev, const float *dh,
                                const float *dh_slabs, int32_t nslabs, int64_t slab_stride, const float *dc,
                                const int64_t *seq_len, int32_t t, int32_t B, int32_t H, float *dgates,
                                float *dc_prev, float *dh_carry, void *stream) {
    DS_REQUIRE(acts && c_t && c_prev && dh && dc && seq_len && dgates && dc_prev && dh_carry && nslabs >= 0 &&
                   (nslabs == 0 || dh_slabs),
               "ds_lstm_cell_bwd: bad argument");
    hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(ds::stream_grid((int64_t)B * H, 256)), dim3(256), 0,
                       (hipStream_t)stream, acts, c_t, c_prev, dh, dh_slabs, nslabs, slab_stride, dc, seq_len, t, B,
                       H, dgates, dc_prev, dh_carry);
    return ds::check_launch("ds_lstm_cell_bwd");
}

// Is the descriptor the keys-absent case (the existing entry points' arithmetic, run as their own instantiation)?
static bool ce_desc_is_default(const ds_ce_desc *ce) { return !ce || (ce->label_smoothing == 0.f && !ce->class_weights); }
static bool ce_desc_ok(const ds_ce_desc *ce) { return !ce || (ce->label_smoothing >= 0.f && ce->label_smoothing < 1.f); }

extern "C" int ds_softmax_ce(const float *logits, const int64_t *labels, int32_t B, int32_t C, float grad_scale,
                             const float *grad_scale_dev, float *loss, float *dlogits, void *stream) {
    DS_REQUIRE(logits && labels && B > 0 && C > 0, "ds_softmax_ce: bad argument");
    hipLaunchKernelGGL(softmax_ce_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, labels, B, C, grad_scale,
                       grad_scale_dev, loss, dlogits, 0.f, (const float *)nullptr);
    return ds::check_launch("ds_softmax_ce");
}

extern "C" int ds_softmax_ce_opts(const ds_ce_desc *ce, const float *logits, const int64_t *labels, int32_t B, int32_t C,
                                  float grad_scale, const float *grad_scale_dev, float *loss, float *dlogits, void *stream) {
    DS_REQUIRE(logits && labels && B > 0 && C > 0, "ds_softmax_ce_opts: bad argument");
    DS_REQUIRE(ce_desc_ok(ce), "ds_softmax_ce_opts: label_smoothing is a number in [0, 1)");
    if (ce_desc_is_default(ce))
        hipLaunchKernelGGL(softmax_ce_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, labels, B, C,
                           grad_scale, grad_scale_dev, loss, dlogits, 0.f, (const float *)nullptr);
    else
        hipLaunchKernelGGL(softmax_ce_kernel<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, labels, B, C,
                           grad_scale, grad_scale_dev, loss, dlogits, ce->label_smoothing, ce->class_weights);
    return ds::check_launch("ds_softmax_ce_opts");
}

extern "C" int ds_adam_tf(float *theta, const float *g, float *m, float *v, int64_t n, int64_t n_wd, float wd,
                          float grad_scale, float lr_t, const float *lr_t_dev, float beta1, float beta2, float eps,
                          void *stream) {
    DS_REQUIRE(theta && g && m && v && n > 0 && n_wd >= 0 && n_wd <= n, "ds_adam_tf: bad argument");
    hipLaunchKernelGGL((adam_tf_kernel<kOptAdam, false>), dim3(ds::stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, theta, g, m, v,
                       (float *)nullptr, n, n_wd, wd, grad_scale, lr_t, lr_t_dev, 0.f, (const float *)nullptr, beta1, beta2,
                       eps, 0.f, 0.f);
    return ds::check_launch("ds_adam_tf");
}

extern "C" int ds_adam_tf_ema(float *theta, const float *g, float *m, float *v, float *shadow, int64_t n, int64_t n_wd,
                              float wd, float grad_scale, float lr_t, const float *lr_t_dev, float ema_rate,
                              const float *ema_rate_dev, float beta1, float beta2, float eps, void *stream) {
    DS_REQUIRE(theta && g && m && v && n > 0 && n_wd >= 0 && n_wd <= n, "ds_adam_tf_ema: bad argument");
    DS_REQUIRE(shadow, "ds_adam_tf_ema: null shadow");
    DS_REQUIRE(ema_rate >= 0.f && ema_rate <= 1.f, "ds_adam_tf_ema: ema_rate must lie in [0, 1] (got %g)", (double)ema_rate);
    hipLaunchKernelGGL((adam_tf_kernel<kOptAdam, true>), dim3(ds::stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, theta, g, m, v,
                       shadow, n, n_wd, wd, grad_scale, lr_t, lr_t_dev, ema_rate, ema_rate_dev, beta1, beta2, eps, 0.f, 0.f);
    return ds::check_launch("ds_adam_tf_ema");
}

extern "C" int ds_grad_norms(const float *theta, const float *g, int64_t n, int64_t n_wd, float wd, float grad_scale,
                             const int64_t *segments, int32_t nseg, const int64_t *chunks, int32_t nchunks, int32_t mode,
                             double clip, int32_t skip_nonfinite, double *partials, double *sumsq, float *factors,
                             int32_t *flags, void *stream) {
    DS_REQUIRE(theta && g && n > 0 && n_wd >= 0 && n_wd <= n, "ds_grad_norms: bad argument");
    DS_REQUIRE(segments && chunks && nseg > 0 && nchunks > 0, "ds_grad_norms: empty segment or chunk table");
    DS_REQUIRE(partials && sumsq && factors && flags, "ds_grad_norms: null output");
    DS_REQUIRE(mode >= 0 && mode <= 2, "ds_grad_norms: mode must be 0 (none), 1 (per variable) or 2 (global), not %d", (int)mode);
    DS_REQUIRE(mode == 0 || (clip > 0.0 && clip <= 1.7976931348623157e308),
               "ds_grad_norms: the clipping threshold must be a finite number > 0 (got %g)", clip);
    hipLaunchKernelGGL(grad_norms_stage1, dim3(ds::stream_grid(nchunks, 1)), dim3(256), 0, (hipStream_t)stream, theta, g, n,
                       n_wd, wd, grad_scale, segments, nseg, chunks, nchunks, partials);
    hipLaunchKernelGGL(grad_norms_stage2, dim3(1), dim3(256), 0, (hipStream_t)stream, segments, nseg, nchunks, partials, mode,
                       clip, skip_nonfinite ? 1 : 0, sumsq, factors, flags);
    return ds::check_launch("ds_grad_norms");
}

extern "C" int ds_adam_tf_clipped(float *theta, const float *g, float *m, float *v, int64_t n, int64_t n_wd, float wd,
                                  float grad_scale, float lr_t, const float *lr_t_dev, float beta1, float beta2, float eps,
                                  const int64_t *segments, int32_t nseg, const int64_t *chunks, int32_t nchunks,
                                  const float *factors, int32_t *flags, void *stream) {
    DS_REQUIRE(theta && g && m && v && n > 0 && n_wd >= 0 && n_wd <= n, "ds_adam_tf_clipped: bad argument");
    DS_REQUIRE(segments && chunks && nseg > 0 && nchunks > 0, "ds_adam_tf_clipped: empty segment or chunk table");
    DS_REQUIRE(factors && flags, "ds_adam_tf_clipped: null factors or flags");
    hipLaunchKernelGGL((adam_tf_clipped_kernel<kOptAdam, false>), dim3(ds::stream_grid(nchunks, 1)), dim3(256), 0, (hipStream_t)stream,
                       theta, g, m, v, (float *)nullptr, n, n_wd, wd, grad_scale, lr_t, lr_t_dev, 0.f, (const float *)nullptr,
                       beta1, beta2, eps, 0.f, 0.f, segments, nseg, chunks, nchunks, factors, flags);
    return ds::check_launch("ds_adam_tf_clipped");
}

extern "C" int ds_adam_tf_clipped_ema(float *theta, const float *g, float *m, float *v, float *shadow, int64_t n, int64_t n_wd,
                                      float wd, float grad_scale, float lr_t, const float *lr_t_dev, float ema_rate,
                                      const float *ema_rate_dev, float beta1, float beta2, float eps, const int64_t *segments,
                                      int32_t nseg, const int64_t *chunks, int32_t nchunks, const float *factors,
                                      int32_t *flags, void *stream) {
    DS_REQUIRE(theta && g && m && v && n > 0 && n_wd >= 0 && n_wd <= n, "ds_adam_tf_clipped_ema: bad argument");
    DS_REQUIRE(segments && chunks && nseg > 0 && nchunks > 0, "ds_adam_tf_clipped_ema: empty segment or chunk table");
    DS_REQUIRE(factors && flags, "ds_adam_tf_clipped_ema: null factors or flags");
    DS_REQUIRE(shadow, "ds_adam_tf_clipped_ema: null shadow");
    DS_REQUIRE(ema_rate >= 0.f && ema_rate <= 1.f, "ds_adam_tf_clipped_ema: ema_rate must lie in [0, 1] (got %g)",
               (double)ema_rate);
    hipLaunchKernelGGL((adam_tf_clipped_kernel<kOptAdam, true>), dim3(ds::stream_grid(nchunks, 1)), dim3(256), 0, (hipStream_t)stream,
                       theta, g, m, v, shadow, n, n_wd, wd, grad_scale, lr_t, lr_t_dev, ema_rate, ema_rate_dev, beta1, beta2,
                       eps, 0.f, 0.f, segments, nseg, chunks, nchunks, factors, flags);
    return ds::check_launch("ds_adam_tf_clipped_ema");
}

// One launch of kind KIND: the clipped loop shape when the descriptor carries tables, the plain one otherwise; either with
// the shadow update when it carries a shadow.
template <int KIND>
static void opt_step_launch(const ds_opt_desc *d, float *theta, const float *g, float *slot0, float *slot1, int64_t n,
                            int64_t n_wd, float wd, float grad_scale, bool clipped, hipStream_t stream) {
    const bool ema = d->shadow != nullptr;
    const float rate = ema ? d->ema_rate : 0.f;
    const float *rate_dev = ema ? d->ema_rate_dev : nullptr;
    if (clipped) {
        const dim3 grid(ds::stream_grid(d->nchunks, 1)), block(256);
        if (ema)
            hipLaunchKernelGGL((adam_tf_clipped_kernel<KIND, true>), grid, block, 0, stream, theta, g, slot0, slot1, d->shadow, n,
                               n_wd, wd, grad_scale, d->lr, d->lr_dev, rate, rate_dev, d->b1, d->b2, d->eps, d->momentum, d->rho,
                               d->segments, d->nseg, d->chunks, d->nchunks, d->factors, d->flags);
        else
            hipLaunchKernelGGL((adam_tf_clipped_kernel<KIND, false>), grid, block, 0, stream, theta, g, slot0, slot1,
                               (float *)nullptr, n, n_wd, wd, grad_scale, d->lr, d->lr_dev, 0.f, (const float *)nullptr, d->b1,
                               d->b2, d->eps, d->momentum, d->rho, d->segments, d->nseg, d->chunks, d->nchunks, d->factors,
                               d->flags);
        return;
    }
    const dim3 grid(ds::stream_grid(n, 256)), block(256);
    if (ema)
        hipLaunchKernelGGL((adam_tf_kernel<KIND, true>), grid, block, 0, stream, theta, g, slot0, slot1, d->shadow, n, n_wd, wd,
                           grad_scale, d->lr, d->lr_dev, rate, rate_dev, d->b1, d->b2, d->eps, d->momentum, d->rho);
    else
        hipLaunchKernelGGL((adam_tf_kernel<KIND, false>), grid, block, 0, stream, theta, g, slot0, slot1, (float *)nullptr, n,
                           n_wd, wd, grad_scale, d->lr, d->lr_dev, 0.f, (const float *)nullptr, d->b1, d->b2, d->eps,
                           d->momentum, d->rho);
}

extern "C" int ds_opt_step(const ds_opt_desc *d, float *theta, const float *g, float *slot0, float *slot1, int64_t n,
                           int64_t n_wd, float wd, float grad_scale, void *stream) {
    DS_REQUIRE(d, "ds_opt_step: null descriptor");
    DS_REQUIRE(theta && g && n > 0 && n_wd >= 0 && n_wd <= n, "ds_opt_step: bad argument");
    DS_REQUIRE(d->kind >= DS_OPT_ADAM && d->kind <= DS_OPT_RMSPROP,
               "ds_opt_step: kind must be 0 (adam), 1 (sgd), 2 (momentum) or 3 (rmsprop), not %d", (int)d->kind);
    DS_REQUIRE(d->kind == DS_OPT_SGD || slot0, "ds_opt_step: kind %d needs slot0", (int)d->kind);
    DS_REQUIRE((d->kind != DS_OPT_ADAM && d->kind != DS_OPT_RMSPROP) || slot1, "ds_opt_step: kind %d needs slot1", (int)d->kind);
    const bool clipped = d->segments || d->chunks || d->nseg != 0 || d->nchunks != 0 || d->factors || d->flags;
    if (clipped) {
        DS_REQUIRE(d->segments && d->chunks && d->nseg > 0 && d->nchunks > 0, "ds_opt_step: empty segment or chunk table");
        DS_REQUIRE(d->factors && d->flags, "ds_opt_step: null factors or flags");
    }
    if (d->shadow)
        DS_REQUIRE(d->ema_rate >= 0.f && d->ema_rate <= 1.f, "ds_opt_step: ema_rate must lie in [0, 1] (got %g)",
                   (double)d->ema_rate);
    const hipStream_t s = (hipStream_t)stream;
    switch (d->kind) {
    case DS_OPT_ADAM: opt_step_launch<kOptAdam>(d, theta, g, slot0, slot1, n, n_wd, wd, grad_scale, clipped, s); break;
    case DS_OPT_SGD: opt_step_launch<kOptSgd>(d, theta, g, slot0, slot1, n, n_wd, wd, grad_scale, clipped, s); break;
    case DS_OPT_MOMENTUM: opt_step_launch<kOptMomentum>(d, theta, g, slot0, slot1, n, n_wd, wd, grad_scale, clipped, s); break;
    default: opt_step_launch<kOptRmsprop>(d, theta, g, slot0, slot1, n, n_wd, wd, grad_scale, clipped, s); break;
    }
    return ds::check_launch("ds_opt_step");
}

extern "C" int ds_grad_accumulate(float *acc, float *g, int64_t n, int32_t mode, void *stream) {
    DS_REQUIRE(acc && g, "ds_grad_accumulate: null pointer");
    DS_REQUIRE(n > 0 && n % 4 == 0, "ds_grad_accumulate: n must be a positive multiple of 4 (got %lld)", (long long)n);
    DS_REQUIRE(mode >= 0 && mode <= 2, "ds_grad_accumulate: mode must be 0 (first), 1 (middle) or 2 (last), not %d", (int)mode);
    DS_REQUIRE(((uintptr_t)acc | (uintptr_t)g) % 16 == 0, "ds_grad_accumulate: acc and g must be 16-byte aligned");
    const int64_t n4 = n / 4;
    const dim3 grid(ds::stream_grid(n4, kAccumVecPerBlock)), block(256);
    float4 *a4 = reinterpret_cast<float4 *>(acc), *g4 = reinterpret_cast<float4 *>(g);
    if (mode == 0) hipLaunchKernelGGL(grad_accumulate_kernel<0>, grid, block, 0, (hipStream_t)stream, a4, g4, n4);
    else if (mode == 1) hipLaunchKernelGGL(grad_accumulate_kernel<1>, grid, block, 0, (hipStream_t)stream, a4, g4, n4);
    else hipLaunchKernelGGL(grad_accumulate_kernel<2>, grid, block, 0, (hipStream_t)stream, a4, g4, n4);
    return ds::check_launch("ds_grad_accumulate");
}

extern "C" int ds_sumsq(const float *x, int64_t n, float *scratch, float *out, void *stream) {
    DS_REQUIRE(x && scratch && out && n > 0, "ds_sumsq: bad argument");
    int blocks = ds::stream_grid(n, 256 * 8);
    if (blocks > kSumsqBlocks) blocks = kSumsqBlocks;
    hipLaunchKernelGGL(sumsq_stage1, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, n, scratch);
    hipLaunchKernelGGL(sum_stage2, dim3(1), dim3(256), 0, (hipStream_t)stream, scratch, blocks, out);
    return ds::check_launch("ds_sumsq");
}

// ---- length-sorted batches (ds_seq_sort_desc, ds_permute_rows) ------------------------------------------------------------
// rank of sample i = #{j : len_j > len_i, or len_j == len_i and j < i}: descending length, stable.  One workgroup, B^2 / 256
// comparisons per thread (B = 256: 256) -- the batch is tiny, the point is that nothing leaves the device.
__global__ __launch_bounds__(256) void seq_sort_desc_kernel(const int64_t *seq_len, int B, int T, int *perm, int64_t *len_sorted) {
    extern __shared__ int lens[];
    for (int i = threadIdx.x; i < B; i += 256) {
        const int64_t l = seq_len[i];
        lens[i] = (int)(l < 0 ? 0 : (l > T ? T : l));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < B; i += 256) {
        const int li = lens[i];
        int rank = 0;
        for (int j = 0; j < B; ++j) {
            const int lj = lens[j];
            rank += (lj > li || (lj == li && j < i)) ? 1 : 0;
        }
        perm[rank] = i;
        len_sorted[rank] = li;
    }
}

template <typename E>
__global__ __launch_bounds__(256) void permute_rows_kernel(const E *src, int64_t lds, E *dst, int64_t ldd, const int *perm,
                                                           int rows, int cols, int gather) {
    const int64_t total = (int64_t)rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int r = (int)(i / cols), c = (int)(i - (int64_t)r * cols);
        const int pr = perm[r];
        if (gather) dst[(int64_t)r * ldd + c] = src[(int64_t)pr * lds + c];
        else dst[(int64_t)pr * ldd + c] = src[(int64_t)r * lds + c];
    }
}

extern "C" int ds_seq_sort_desc(const int64_t *seq_len, int32_t B, int32_t T, int32_t *perm, int64_t *len_sorted, void *stream) {
    DS_REQUIRE(seq_len && perm && len_sorted && B > 0 && B <= 4096 && T > 0, "ds_seq_sort_desc: bad argument (1 <= B <= 4096)");
    hipLaunchKernelGGL(seq_sort_desc_kernel, dim3(1), dim3(256), (size_t)B * sizeof(int), (hipStream_t)stream, seq_len, B, T, perm,
                       len_sorted);
    return ds::check_launch("ds_seq_sort_desc");
}

extern "C" int ds_permute_rows(const void *src, int64_t lds, void *dst, int64_t ldd, const int32_t *perm, int32_t rows, int32_t cols,
                               int32_t elem_bytes, int32_t gather, void *stream) {
    DS_REQUIRE(src && dst && perm && rows > 0 && cols > 0 && lds >= cols && ldd >= cols && (elem_bytes == 4 || elem_bytes == 8),
               "ds_permute_rows: bad argument (elem_bytes 4 or 8)");
    const int grid = ds::stream_grid((int64_t)rows * cols, 256);
    if (elem_bytes == 4)
        hipLaunchKernelGGL(permute_rows_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float *)src, lds,
                           (float *)dst, ldd, perm, rows, cols, gather);
    else
        hipLaunchKernelGGL(permute_rows_kernel<int64_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const int64_t *)src, lds,
                           (int64_t *)dst, ldd, perm, rows, cols, gather);
    return ds::check_launch("ds_permute_rows");
}

extern "C" int ds_colsum(const float *x, int64_t M, int32_t C, int32_t ld, float *scratch, float *out, void *stream) {
    DS_REQUIRE(x && scratch && out && M > 0 && C > 0 && ld >= C, "ds_colsum: bad argument");
    int RS = (int)((M + 63) / 64);
    if (RS > 64) RS = 64;
    const int rps = (int)((M + RS - 1) / RS);
    if (RS <= 8) {
        hipLaunchKernelGGL(colsum_small_kernel, dim3((C + 63) / 64), dim3(256), 0, (hipStream_t)stream, x, M, C, ld, rps, RS, out);
        return ds::check_launch("ds_colsum");
    }
    hipLaunchKernelGGL(colsum_stage1, dim3((C + 63) / 64, RS), dim3(256), 0, (hipStream_t)stream, x, M, C, ld, rps,
                       scratch);
    hipLaunchKernelGGL(colsum_stage2, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, scratch, RS, C, out);
    return ds::check_launch("ds_colsum");
}

// out[m][n] = epilogue(sum_s slabs[s][m][n]): the second half of a split-K GEMM (ds_conv_igemm with splits > 1 writes slab s at
// z + s * z_split_stride).  The M <= 512 GEMMs of the heads are ONE row tile or two: a single launch walks K = 512 ... 1024
// serially in a handful of workgroups (40-57 us each, on the chain between the towers' forward and backward passes);
// split eight ways and combined here in a fixed order (deterministic) they take a third of that.
__global__ __launch_bounds__(256) void slab_epilogue_kernel(const float *slabs, int splits, int64_t slab_stride, int lds,
                                                            int64_t M, int N, float *out, int ldo, const float *bias,
                                                            const float *mask, int ldmask, int flags) {
    const int64_t total = M * N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t m = i / N;
        const int n = (int)(i - m * N);
        float v = 0.f;
        for (int k = 0; k < splits; ++k) v += slabs[(int64_t)k * slab_stride + m * lds + n];
        if (flags & DS_EPI_BIAS) v += bias[n];
        const int64_t o = m * ldo + n;
        if (flags & DS_EPI_ACCUM) v += out[o];
        if (flags & DS_EPI_MASK) v = mask[m * ldmask + n] > 0.f ? v : 0.f;
        if (flags & DS_EPI_RELU) v = fmaxf(v, 0.f);
        out[o] = v;
    }
}

extern "C" int ds_slab_epilogue(const float *slabs, int32_t splits, int64_t slab_stride, int32_t lds, int64_t M, int32_t N,
                                float *out, int32_t ldo, const float *bias, const float *mask, int32_t ldmask, int32_t flags,
                                void *stream) {
    DS_REQUIRE(slabs && out && splits >= 1 && M > 0 && N > 0 && lds >= N && ldo >= N, "ds_slab_epilogue: bad argument");
    DS_REQUIRE((flags & ~(DS_EPI_BIAS | DS_EPI_ACCUM | DS_EPI_MASK | DS_EPI_RELU)) == 0 && (!(flags & DS_EPI_BIAS) || bias) &&
                   (!(flags & DS_EPI_MASK) || (mask && ldmask >= N)),
               "ds_slab_epilogue: flags are BIAS / ACCUM / MASK / RELU (with their operands)");
    hipLaunchKernelGGL(slab_epilogue_kernel, dim3(ds::stream_grid(M * N, 256)), dim3(256), 0, (hipStream_t)stream, slabs, splits,
                       slab_stride, lds, M, N, out, ldo, bias, mask, ldmask, flags);
    return ds::check_launch("ds_slab_epilogue");
}

// ---- the combines of several split-K GEMMs as ONE launch (ds_slab_epilogue_group) -----------------------------------------
// Combine i is slab_epilogue_kernel's arithmetic on its own slabs, with two extensions the joint head needs:
//   * pre_slabs: the DS_EPI_ACCUM operand is not read from `out` but formed here, sum of pre_slabs in index order from 0 --
//     what a plain ds_slab_epilogue of those slabs into `out` would have left there (W_fc's image half under its text half);
//   * out2: columns [n_split, N) go to out2[m * ldo2 + n - n_split] (one dgrad through W_fc, the image and the text gradient).
constexpr int kCombineMax = 4;
struct SlabCombineParams {
    ds_slab_combine op[kCombineMax];
    int wg_end[kCombineMax];      // first workgroup past combine i
    int count;
};

__global__ __launch_bounds__(256) void slab_epilogue_group_kernel(const SlabCombineParams g) {
    const int id = (int)blockIdx.x;
    int q = 0;
    while (q + 1 < g.count && id >= g.wg_end[q]) ++q;
    const int wg0 = q ? g.wg_end[q - 1] : 0;
    const ds_slab_combine &c = g.op[q];
    const int64_t total = c.M * c.N, step = (int64_t)(g.wg_end[q] - wg0) * 256;
    const int N = c.N, flags = c.flags;
    for (int64_t i = (int64_t)(id - wg0) * 256 + threadIdx.x; i < total; i += step) {
        const int64_t m = i / N;
        const int n = (int)(i - m * N);
        float v = 0.f;
        for (int k = 0; k < c.splits; ++k) v += c.slabs[(int64_t)k * c.slab_stride + m * c.lds + n];
        if (flags & DS_EPI_BIAS) v += c.bias[n];
        float *const o = (c.out2 && n >= c.n_split) ? c.out2 + m * c.ldo2 + (n - c.n_split) : c.out + m * c.ldo + n;
        if (flags & DS_EPI_ACCUM) {
            if (c.pre_slabs) {
                float u = 0.f;
                for (int k = 0; k < c.pre_splits; ++k) u += c.pre_slabs[(int64_t)k * c.pre_slab_stride + m * c.pre_lds + n];
                v += u;
            } else {
                v += *o;
            }
        }
        if (flags & DS_EPI_MASK) v = c.mask[m * c.ldmask + n] > 0.f ? v : 0.f;
        if (flags & DS_EPI_RELU) v = fmaxf(v, 0.f);
        *o = v;
    }
}

extern "C" int ds_slab_epilogue_group(const ds_slab_combine *ops, int32_t count, void *stream) {
    DS_REQUIRE(ops && count >= 1 && count <= kCombineMax, "ds_slab_epilogue_group: 1..%d combines", kCombineMax);
    SlabCombineParams g{};
    g.count = count;
    int wgs = 0;
    for (int i = 0; i < count; ++i) {
        const ds_slab_combine &c = ops[i];
        DS_REQUIRE(c.slabs && c.out && c.splits >= 1 && c.M > 0 && c.N > 0 && c.lds >= c.N, "ds_slab_epilogue_group: bad argument (combine %d)", i);
        DS_REQUIRE((c.flags & ~(DS_EPI_BIAS | DS_EPI_ACCUM | DS_EPI_MASK | DS_EPI_RELU)) == 0 && (!(c.flags & DS_EPI_BIAS) || c.bias) &&
                       (!(c.flags & DS_EPI_MASK) || (c.mask && c.ldmask >= c.N)),
                   "ds_slab_epilogue_group: flags are BIAS / ACCUM / MASK / RELU (with their operands)");
        DS_REQUIRE(!c.pre_slabs || ((c.flags & DS_EPI_ACCUM) && c.pre_splits >= 1 && c.pre_lds >= c.N),
                   "ds_slab_epilogue_group: pre_slabs is the DS_EPI_ACCUM operand (pre_splits >= 1, pre_lds >= N)");
        if (c.out2)
            DS_REQUIRE(c.n_split > 0 && c.n_split < c.N && c.ldo >= c.n_split && c.ldo2 >= c.N - c.n_split,
                       "ds_slab_epilogue_group: out2 takes columns [n_split, N), 0 < n_split < N");
        else
            DS_REQUIRE(c.ldo >= c.N, "ds_slab_epilogue_group: ldo below N (combine %d)", i);
        g.op[i] = c;
        wgs += ds::stream_grid(c.M * c.N, 256);
        g.wg_end[i] = wgs;
    }
    hipLaunchKernelGGL(slab_epilogue_group_kernel, dim3(wgs), dim3(256), 0, (hipStream_t)stream, g);
    return ds::check_launch("ds_slab_epilogue_group");
}

// The combine of the W_softmax GEMM's slabs (bias added: the logits) going straight on to the cross entropy and its gradient:
// one workgroup, as ds_softmax_ce is -- thread t combines rows t and t + 256, stores them, and runs ds_softmax_ce's own
// arithmetic on them (softmax_ce_workgroup), so logits, loss and dlogits are the bits of ds_slab_epilogue + ds_softmax_ce.
template <bool OPTS>
__global__ __launch_bounds__(256) void slab_epilogue_ce_kernel(const float *slabs, int splits, int64_t slab_stride, int lds,
                                                               int M, int N, float *logits, const float *bias,
                                                               const int64_t *labels, float grad_scale,
                                                               const float *grad_scale_dev, float *loss, float *dlogits,
                                                               float eps, const float *cw) {
    __shared__ float red[256];
    for (int m = threadIdx.x; m < M; m += 256) {
        for (int n = 0; n < N; ++n) {
            float v = 0.f;
            for (int k = 0; k < splits; ++k) v += slabs[(int64_t)k * slab_stride + (int64_t)m * lds + n];
            if (bias) v += bias[n];
            logits[(int64_t)m * N + n] = v;
        }
    }
    softmax_ce_workgroup<OPTS>(logits, labels, M, N, grad_scale, grad_scale_dev, loss, dlogits, red, eps, cw);
}

extern "C" int ds_slab_epilogue_ce(const float *slabs, int32_t splits, int64_t slab_stride, int32_t lds, int32_t M, int32_t N,
                                   float *logits, const float *bias, const int64_t *labels, float grad_scale,
                                   const float *grad_scale_dev, float *loss, float *dlogits, void *stream) {
    DS_REQUIRE(slabs && logits && labels && splits >= 1 && lds >= N, "ds_slab_epilogue_ce: bad argument");
    DS_REQUIRE(M > 0 && M <= 512 && N > 0 && N <= 32, "ds_slab_epilogue_ce: M <= 512 rows of N <= 32 logits (packed, row stride N)");
    hipLaunchKernelGGL(slab_epilogue_ce_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, slabs, splits, slab_stride, lds,
                       M, N, logits, bias, labels, grad_scale, grad_scale_dev, loss, dlogits, 0.f, (const float *)nullptr);
    return ds::check_launch("ds_slab_epilogue_ce");
}

extern "C" int ds_slab_epilogue_ce_opts(const ds_ce_desc *ce, const float *slabs, int32_t splits, int64_t slab_stride,
                                        int32_t lds, int32_t M, int32_t N, float *logits, const float *bias,
                                        const int64_t *labels, float grad_scale, const float *grad_scale_dev, float *loss,
                                        float *dlogits, void *stream) {
    DS_REQUIRE(slabs && logits && labels && splits >= 1 && lds >= N, "ds_slab_epilogue_ce_opts: bad argument");
    DS_REQUIRE(M > 0 && M <= 512 && N > 0 && N <= 32,
               "ds_slab_epilogue_ce_opts: M <= 512 rows of N <= 32 logits (packed, row stride N)");
    DS_REQUIRE(ce_desc_ok(ce), "ds_slab_epilogue_ce_opts: label_smoothing is a number in [0, 1)");
    if (ce_desc_is_default(ce))
        hipLaunchKernelGGL(slab_epilogue_ce_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, slabs, splits, slab_stride,
                           lds, M, N, logits, bias, labels, grad_scale, grad_scale_dev, loss, dlogits, 0.f,
                           (const float *)nullptr);
    else
        hipLaunchKernelGGL(slab_epilogue_ce_kernel<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, slabs, splits, slab_stride,
                           lds, M, N, logits, bias, labels, grad_scale, grad_scale_dev, loss, dlogits, ce->label_smoothing,
                           ce->class_weights);
    return ds::check_launch("ds_slab_epilogue_ce_opts");
}

extern "C" int ds_copy2d(const float *src, int32_t lds, float *dst, int32_t ldd, int64_t rows, int32_t cols,
                         void *stream) {
    DS_REQUIRE(src && dst && rows > 0 && cols > 0, "ds_copy2d: bad argument");
    hipLaunchKernelGGL(copy2d_kernel, dim3(ds::stream_grid(rows * cols, 256)), dim3(256), 0, (hipStream_t)stream, src,
                       lds, dst, ldd, rows, cols);
    return ds::check_launch("ds_copy2d");
}

extern "C" int ds_pad_channels(const float *src, int32_t cs, float *dst, int32_t cd, int64_t pixels, void *stream) {
    DS_REQUIRE(src && dst && cs > 0 && cd >= cs && pixels > 0, "ds_pad_channels: bad argument");
    hipLaunchKernelGGL(pad_channels_kernel, dim3(ds::stream_grid(pixels * cd, 256)), dim3(256), 0, (hipStream_t)stream,
                       src, cs, dst, cd, pixels);
    return ds::check_launch("ds_pad_channels");
}

extern "C" int ds_fill(float *dst, int64_t n, float value, void *stream) {
    DS_REQUIRE(dst && n > 0, "ds_fill: bad argument");
    hipLaunchKernelGGL(fill_kernel, dim3(ds::stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, dst, n, value);
    return ds::check_launch("ds_fill");
}
