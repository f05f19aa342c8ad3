// The per-video, temporal part of the evaluation on the device (data/PW3D/dataset.py:383-415, which the reference keeps commented out):
//   gator_one_euro_f32    : lib/smooth_utils.smooth_pose, a one-euro filter along every channel of every video, in ONE launch;
//   gator_sequence_errors : per frame the acceleration error of the triple it starts (lib/coord_utils.py:194-222), the mean joint
//                           distance and the same after the similarity fit (lib/coord_utils.py:127-149), then per video their
//                           fixed-order sums -- two launches.
// Frames of V videos lie one video after another; seg_start [V+1] (int64, device) holds each video's first frame and, last, F.
// Nothing is atomic and every sum has a fixed order: a result is the same bits from run to run, whatever lies around it.
//
// The filter is a strictly sequential chain in T: the cutoff of step t depends on the FILTERED derivative of step t, which depends on
// the filtered value of step t-1, so there is no associative operator to scan with.  Each step carries a dependent fp64 division (two
// when dt != 1); the kernel's time is T_max x that latency whatever C and V.  What does not depend on the chain -- the loads -- runs kPrefetch
// frames ahead in a register ring.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "procrustes.h"

namespace gator {
namespace {

constexpr int kEuroThreads = 64;      // one lane per (video, channel); consecutive lanes take consecutive channels of one video
constexpr int kPrefetch = 8;          // PF: frames whose loads are in flight ahead of the chain (gator_amd/temporal.py: PREFETCH)
constexpr int kSeqThreads = 64;       // k_seq_errors: one lane per frame, the LDS point sets (procrustes.h: kPtsLds) have 64 columns

// lib/smooth_utils.py:27-46 as smooth_pose drives it (:49-72), step for step in fp64: x_hat[0] = x[0], dx_prev = 0, t_e = dt;
//   a_d = sf(t_e, d_cutoff); dx = (x - x_prev) / t_e; dx_hat = a_d dx + (1 - a_d) dx_prev;
//   cutoff = min_cutoff + beta |dx_hat|; a = sf(t_e, cutoff); x_hat = a x + (1 - a) x_prev;      sf(t_e, c) = r / (r + 1), r = 2 pi c t_e.
// Every product and sum is rounded on its own, as numpy rounds it: an a * x + b contracted into one FMA differs in the last bit.
// One step of the chain.  UnitDt: dt == 1, where (x - x_prev) / 1.0 is exact and the division is left out.
template <bool UnitDt>
__device__ __forceinline__ double euro_step(double xt, double& x_prev, double& dx_prev, double a_d, double b_d, double min_cutoff, double beta,
                                            double two_pi, double dt) {
#pragma clang fp contract(off)
    const double d = xt - x_prev;
    const double dx = UnitDt ? d : d / dt;
    const double dx_hat = a_d * dx + b_d * dx_prev;
    const double cutoff = min_cutoff + beta * fabs(dx_hat);
    const double r = two_pi * cutoff * dt;              // left to right
    const double a = r / (r + 1.0);
    const double x_hat = a * xt + (1.0 - a) * x_prev;
    dx_prev = dx_hat;
    x_prev = x_hat;
    return x_hat;
}

// blockIdx.x = video * chunks + chunk: V is bounded by the x limit of a grid, not by its y limit.
template <typename Out, bool UnitDt>
__global__ __launch_bounds__(kEuroThreads) void k_one_euro(const float* __restrict__ x, const int64_t* __restrict__ seg_start, int C, int chunks,
                                                           double min_cutoff, double beta, double d_cutoff, double dt, Out* __restrict__ out) {
#pragma clang fp contract(off)
    const int v = blockIdx.x / chunks;
    const int c = (blockIdx.x - v * chunks) * kEuroThreads + threadIdx.x;
    if (c >= C) return;
    const int64_t s = seg_start[v], T = seg_start[v + 1] - s;
    const float* xp = x + (size_t)s * C + c;
    Out* op = out + (size_t)s * C + c;

    const double two_pi = 2.0 * 3.141592653589793;      // 2 * math.pi: exact doubling
    const double r_d = two_pi * d_cutoff * dt;          // left to right
    const double a_d = r_d / (r_d + 1.0), b_d = 1.0 - a_d;

    // ring[k] holds frame t + k of the group that starts at t.  A load past the video's end is clamped to its last frame: always a
    // valid address, no branch in the group's body, and the value is never used.
    const int64_t last = T - 1;
    float ring[kPrefetch];
#pragma unroll
    for (int k = 0; k < kPrefetch; ++k) ring[k] = xp[(size_t)(1 + k < last ? 1 + k : last) * C];
    double x_prev = (double)xp[0], dx_prev = 0.0;       // the first frame is copied
    op[0] = (Out)x_prev;

    int64_t t = 1;
    for (; t + kPrefetch <= T; t += kPrefetch) {         // whole groups: straight-line code, the loads kPrefetch frames ahead of their use
#pragma unroll
        for (int k = 0; k < kPrefetch; ++k) {
            const double xt = (double)ring[k];
            const int64_t nt = t + k + kPrefetch;
            ring[k] = xp[(size_t)(nt < last ? nt : last) * C];
            op[(size_t)(t + k) * C] = (Out)euro_step<UnitDt>(xt, x_prev, dx_prev, a_d, b_d, min_cutoff, beta, two_pi, dt);
        }
    }
#pragma unroll
    for (int k = 0; k < kPrefetch - 1; ++k)              // the last, partial group: its frames are in the ring already
        if (t + k < T) op[(size_t)(t + k) * C] = (Out)euro_step<UnitDt>((double)ring[k], x_prev, dx_prev, a_d, b_d, min_cutoff, beta, two_pi, dt);
}

// rows [F,3] fp64.  Frame i of video v (frames s .. e-1):
//   0  i + 2 < e and frames i, i+1, i+2 valid: mean over joints of |(p_i - 2 p_i+1 + p_i+2) - (g_i - 2 g_i+1 + g_i+2)|; else NaN
//   1  mean over joints of |p_i - g_i|
//   2  the same after the similarity fit of p_i onto g_i
template <typename Pred>
__global__ __launch_bounds__(kSeqThreads) void k_seq_errors(const Pred* __restrict__ P, const float* __restrict__ G, const uint8_t* __restrict__ valid,
                                                            const int64_t* __restrict__ seg_start, int V, int64_t F, int ne, double* __restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * kSeqThreads + threadIdx.x;
    if (i >= F) return;
    extern __shared__ double pts_lds[];                  // [2][kMaxPts][3][kSeqThreads]
    const Pts pa{pts_lds, (int)threadIdx.x, kSeqThreads}, pt{pts_lds + (size_t)kMaxPts * 3 * kSeqThreads, (int)threadIdx.x, kSeqThreads};
    // the video of frame i: the last v with seg_start[v] <= i (every video has at least one frame, so the starts strictly increase)
    int lo = 0, hi = V;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_start[mid] <= i) lo = mid; else hi = mid;
    }
    const int64_t e = seg_start[lo + 1];
    const int n3 = ne * 3;
    const Pred* p = P + (size_t)i * n3;
    const float* g = G + (size_t)i * n3;
    const bool triple = i + 2 < e && (!valid || (valid[i] && valid[i + 1] && valid[i + 2]));
    double acc = 0.0, e1 = 0.0;
    for (int j = 0; j < ne; ++j) {
        double d2 = 0.0, a2 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double pk = (double)p[j * 3 + k], gk = (double)g[j * 3 + k];
            pa(j, k) = pk; pt(j, k) = gk;
            d2 += (pk - gk) * (pk - gk);
            if (triple) {
                const double ap = (pk - 2.0 * (double)p[n3 + j * 3 + k]) + (double)p[2 * n3 + j * 3 + k];
                const double ag = (gk - 2.0 * (double)g[n3 + j * 3 + k]) + (double)g[2 * n3 + j * 3 + k];
                a2 += (ap - ag) * (ap - ag);
            }
        }
        e1 += sqrt(d2);
        acc += sqrt(a2);
    }
    double c, R[3][3], tr[3];
    rigid_fit(pa, pt, ne, c, R, tr);
    const double e2 = aligned_error<false>(pa, pt, ne, c, R, tr);
    double* o = rows + (size_t)i * 3;
    o[0] = triple ? acc / ne : __builtin_nan("");
    o[1] = e1 / ne;
    o[2] = e2 / ne;
}

// sums [V,6] fp64: the sums of the three columns over the video (column 0 over its non-NaN rows), the count of those rows, the frame
// count, 0.  One wave per video: lane l adds rows l, l + 64, ... in order, then an xor butterfly (a + b == b + a bit for bit).
__global__ __launch_bounds__(64) void k_seq_reduce(const double* __restrict__ rows, const int64_t* __restrict__ seg_start, double* __restrict__ sums) {
    const int v = blockIdx.x;
    const int64_t s = seg_start[v], e = seg_start[v + 1];
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = s + threadIdx.x; i < e; i += 64) {
        const double r0 = rows[(size_t)i * 3];
        if (r0 == r0) { a[0] += r0; a[3] += 1.0; }
        a[1] += rows[(size_t)i * 3 + 1];
        a[2] += rows[(size_t)i * 3 + 2];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = wave_sum(a[k]);
    if (threadIdx.x == 0) {
        double* o = sums + (size_t)v * 6;
        o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3]; o[4] = (double)(e - s); o[5] = 0.0;
    }
}

}  // namespace
}  // namespace gator

extern "C" int gator_one_euro_f32(const float* x, const int64_t* seg_start, int64_t n_frames, int32_t n_videos, int32_t n_channels,
                                  double min_cutoff, double beta, double d_cutoff, double dt, int32_t out_f64, void* out, void* stream) {
    using namespace gator;
    if (!x || !seg_start || !out) return fail(GATOR_EINVAL, "gator_one_euro_f32: null input, seg_start or output");
    if (n_frames <= 0 || n_videos <= 0 || n_channels <= 0 || n_videos > n_frames)
        return fail(GATOR_EINVAL, "gator_one_euro_f32: %lld frames, %d videos, %d channels (each >= 1, a video has a frame)", (long long)n_frames, n_videos, n_channels);
    if (!(dt > 0.0)) return fail(GATOR_EINVAL, "gator_one_euro_f32: dt must be positive");
    const int chunks = (n_channels + kEuroThreads - 1) / kEuroThreads;
    if ((int64_t)chunks * n_videos > 0x7fffffffLL) return fail(GATOR_EINVAL, "gator_one_euro_f32: videos x channel chunks exceed a grid");
    const dim3 grid((unsigned)(chunks * n_videos));
    const hipStream_t st = (hipStream_t)stream;
    const bool unit_dt = dt == 1.0;
    if (out_f64 && unit_dt)
        k_one_euro<double, true><<<grid, kEuroThreads, 0, st>>>(x, seg_start, n_channels, chunks, min_cutoff, beta, d_cutoff, dt, (double*)out);
    else if (out_f64)
        k_one_euro<double, false><<<grid, kEuroThreads, 0, st>>>(x, seg_start, n_channels, chunks, min_cutoff, beta, d_cutoff, dt, (double*)out);
    else if (unit_dt)
        k_one_euro<float, true><<<grid, kEuroThreads, 0, st>>>(x, seg_start, n_channels, chunks, min_cutoff, beta, d_cutoff, dt, (float*)out);
    else
        k_one_euro<float, false><<<grid, kEuroThreads, 0, st>>>(x, seg_start, n_channels, chunks, min_cutoff, beta, d_cutoff, dt, (float*)out);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

extern "C" int gator_sequence_errors(const void* pred, int32_t pred_f64, const float* gt, const uint8_t* valid, const int64_t* seg_start,
                                     int64_t n_frames, int32_t n_videos, int32_t n_eval, double* rows, double* video_sums, void* stream) {
    using namespace gator;
    if (!pred || !gt || !seg_start || !rows || !video_sums) return fail(GATOR_EINVAL, "gator_sequence_errors: null input, seg_start or output");
    if (n_frames <= 0 || n_videos <= 0 || n_videos > n_frames)
        return fail(GATOR_EINVAL, "gator_sequence_errors: %lld frames, %d videos (each >= 1, a video has a frame)", (long long)n_frames, n_videos);
    if (n_eval < 3 || n_eval > kMaxPts) return fail(GATOR_EINVAL, "gator_sequence_errors: 3..32 evaluation joints");
    const int64_t blocks = (n_frames + kSeqThreads - 1) / kSeqThreads;
    if (blocks > 0x7fffffffLL) return fail(GATOR_EINVAL, "gator_sequence_errors: too many frames for a grid");
    static bool raised_f64_[64] = {}, raised_f32_[64] = {};
    if (pred_f64) {
        if (int rc = raise_pts_lds((const void*)k_seq_errors<double>, raised_f64_)) return rc;
        k_seq_errors<double><<<(unsigned)blocks, kSeqThreads, kPtsLds, (hipStream_t)stream>>>((const double*)pred, gt, valid, seg_start, n_videos, n_frames,
                                                                                           n_eval, rows);
    } else {
        if (int rc = raise_pts_lds((const void*)k_seq_errors<float>, raised_f32_)) return rc;
        k_seq_errors<float><<<(unsigned)blocks, kSeqThreads, kPtsLds, (hipStream_t)stream>>>((const float*)pred, gt, valid, seg_start, n_videos, n_frames,
                                                                                          n_eval, rows);
    }
    GATOR_HIP_CHECK(hipGetLastError());
    k_seq_reduce<<<(unsigned)n_videos, 64, 0, (hipStream_t)stream>>>(rows, seg_start, video_sums);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}
