// ds_eval_metrics_update: the streaming evaluation metrics of one batch of logits -- confusion matrix, rank histogram
// (top-k accuracy), the counters and the cross-entropy sum -- added to accumulators that stay on the device, so that an
// evaluation loop reads nothing back until it is over.
//
//   eval_metrics_kernel<G>   G lanes own one row: G = 1 up to kNarrowC columns (C = 15: a row is 60 bytes, a workgroup of 256
//                            rows reads one contiguous 15 KB range), G = 64 above (C = 1000: a wave walks the row with
//                            coalesced 256-byte loads; four rows per wave, 16 per workgroup).  Pass 1 finds the maximum,
//                            its lowest index and any non-finite value; pass 2 (the row is in L1 by then) sums
//                            exp(z - max) in double and counts the label's rank.  A group combines with xor butterflies:
//                            every lane ends with the same bits, whatever the order.
//                            Integer bins: a row yields at most two bin indices (confusion or a counter, and its rank bin).
//                            They are staged in LDS -- C * C bins do not fit there at C = 1000, the rows' indices always do --
//                            and combined per workgroup: the first holder of an index counts its occurrences and makes the
//                            ONE global add of that bin.  Integer adds commute, so the counts do not depend on the order.
//                            Loss: the workgroup's rows are summed in a fixed tree (butterfly per wave, then w0 + w1 + w2 +
//                            w3) into partials[blockIdx.x].
//   eval_metrics_loss_sum    one wave: lane l adds partials l, l + 64, ... in index order, a butterfly, loss_sum[0] += the
//                            batch's sum.  No float atomic, no hand-off between workgroups: stream order is the only fence.
#include "ds_common.h"

namespace {

constexpr int kNarrowC = 32;          // up to here a lane owns a row
constexpr int kWideRows = 16;         // rows per workgroup of the wave-per-row form
constexpr int kMaxB = 65536, kMaxC = 1024;

inline int rows_per_block(int C) { return C <= kNarrowC ? 256 : kWideRows; }

template <int G>
__global__ __launch_bounds__(256) void eval_metrics_kernel(const float *__restrict__ logits, int ldl,
                                                           const int64_t *__restrict__ labels, int B, int C,
                                                           unsigned long long *__restrict__ counts,
                                                           double *__restrict__ partials) {
    constexpr int RB = G == 1 ? 256 : kWideRows;       // rows per workgroup
    constexpr int RPG = RB / (256 / G);                // rows per lane group
    __shared__ int keys[2][RB];
    __shared__ double wsum[4];
    const int t = threadIdx.x, g = t % G, grp = t / G;
    const int bins = C * C;
    double loss = 0.0;

    for (int r = 0; r < RPG; ++r) {
        const int slot = grp * RPG + r;
        const int64_t row = (int64_t)blockIdx.x * RB + slot;
        int k0 = -1, k1 = -1;
        if (row < B) {                                  // uniform over the lane group
            const float *z = logits + row * (int64_t)ldl;
            const int64_t y = labels[row];
            float m = -INFINITY;
            int am = C, nonfinite = 0;
            for (int j = g; j < C; j += G) {
                const float v = z[j];
                nonfinite |= (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
                if (v > m) {                            // strict: a lane keeps its lowest index
                    m = v;
                    am = j;
                }
            }
#pragma unroll
            for (int o = G >> 1; o > 0; o >>= 1) {
                const float om = __shfl_xor(m, o);
                const int oa = __shfl_xor(am, o);
                nonfinite |= __shfl_xor(nonfinite, o);
                if (om > m || (om == m && oa < am)) {
                    m = om;
                    am = oa;
                }
            }
            if (nonfinite) {
                k0 = bins + C + 1;
            } else if (y < 0 || y >= C) {               // no address is formed from such a label
                k0 = bins + C + 2;
            } else {
                const int yi = (int)y;
                const float zy = z[yi];
                double s = 0.0;
                int rank = 0;
                for (int j = g; j < C; j += G) {
                    const float v = z[j];
                    s += exp((double)v - (double)m);
                    rank += (v > zy || (v == zy && j < yi)) ? 1 : 0;
                }
#pragma unroll
                for (int o = G >> 1; o > 0; o >>= 1) {
                    s += __shfl_xor(s, o);
                    rank += __shfl_xor(rank, o);
                }
                k0 = yi * C + am;
                k1 = bins + rank;
                if (g == 0) loss += log(s) + ((double)m - (double)zy);
            }
        }
        if (g == 0) {
            keys[0][slot] = k0;
            keys[1][slot] = k1;
        }
    }

    loss = ds::wave_sum_f64(loss);
    if ((t & 63) == 0) wsum[t >> 6] = loss;
    __syncthreads();
    if (t == 255) {                                     // a thread without a row in the wide form
        partials[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        int counted = 0;                                // n: the rows that have a rank
        for (int j = 0; j < RB; ++j) counted += keys[1][j] >= 0;
        if (counted) atomicAdd(counts + bins + C, (unsigned long long)counted);
    }
    if (t < RB) {
#pragma unroll
        for (int cls = 0; cls < 2; ++cls) {
            const int key = keys[cls][t];
            if (key < 0) continue;
            bool first = true;
            int cnt = 0;
            for (int j = 0; j < RB; ++j) {
                if (keys[cls][j] == key) {
                    first = first && j >= t;
                    ++cnt;
                }
            }
            if (first) atomicAdd(counts + key, (unsigned long long)cnt);
        }
    }
}

__global__ __launch_bounds__(64) void eval_metrics_loss_sum(const double *__restrict__ partials, int P,
                                                           double *__restrict__ loss_sum) {
    double s = 0.0;
    for (int i = threadIdx.x; i < P; i += 64) s += partials[i];
    s = ds::wave_sum_f64(s);
    if (threadIdx.x == 0) loss_sum[0] += s;
}

}  // namespace

extern "C" int ds_eval_metrics_workspace(int32_t B, int32_t C) {
    DS_REQUIRE(B >= 1 && B <= kMaxB && C >= 1 && C <= kMaxC, "ds_eval_metrics_workspace: B must be in [1, 65536], C in [1, 1024]");
    const int rb = rows_per_block(C);
    return (B + rb - 1) / rb * (int)sizeof(double);
}

extern "C" int ds_eval_metrics_update(const float *logits, int32_t ldl, const int64_t *labels, int32_t B, int32_t C,
                                      int64_t *counts, double *loss_sum, void *scratch, void *stream) {
    DS_REQUIRE(logits && labels && counts && loss_sum && scratch, "ds_eval_metrics_update: null pointer");
    DS_REQUIRE(B >= 1 && B <= kMaxB, "ds_eval_metrics_update: B must be in [1, 65536]");
    DS_REQUIRE(C >= 1 && C <= kMaxC, "ds_eval_metrics_update: C must be in [1, 1024]");
    DS_REQUIRE(ldl >= C, "ds_eval_metrics_update: ldl < C");
    DS_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)labels & 7) == 0 && ((uintptr_t)counts & 7) == 0 &&
                   ((uintptr_t)loss_sum & 7) == 0 && ((uintptr_t)scratch & 7) == 0,
               "ds_eval_metrics_update: logits must be 4-byte aligned, labels, counts, loss_sum and scratch 8-byte");
    const int rb = rows_per_block(C), blocks = (B + rb - 1) / rb;
    unsigned long long *bins = reinterpret_cast<unsigned long long *>(counts);
    double *partials = static_cast<double *>(scratch);
    if (C <= kNarrowC)
        hipLaunchKernelGGL(eval_metrics_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, ldl, labels, B, C,
                           bins, partials);
    else
        hipLaunchKernelGGL(eval_metrics_kernel<64>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, ldl, labels, B, C,
                           bins, partials);
    hipLaunchKernelGGL(eval_metrics_loss_sum, dim3(1), dim3(64), 0, (hipStream_t)stream, partials, blocks, loss_sum);
    return ds::check_launch("ds_eval_metrics_update");
}
