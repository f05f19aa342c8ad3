// The detector noise of the training input (include/gator_hip.h: gator_preprocess_noise_f32; DESIGN.md "Detector noise"): the datasets'
// replace_joint_img step (data/Human36M/dataset.py:369-389, 421-453) between the crop affine and the flip, on the device.
//   k_noise_crop        one lane per sample: the 2D chain of joints2d.h up to the float32 crop joints, the box area of synthesize_pose,
//                       and what needs no candidates -- generate_syn_error (stats) and the detections branch
//   k_noise_candidates  lib/noise_utils.synthesize_pose: one wave per symmetric pair (or unpaired joint) of a sample, a joint's
//                       candidates spread over the lanes, accepted ones counted with ballots
//   k_noise_finish      one lane per sample: flip_2d_joint on the float32 joints, /[W,H], the standardisation
// fp64 where the reference has it; the build disables contracted multiply-adds for every source (gator_amd/build.py: FLAGS).
#include <hip/hip_runtime.h>

#include "handle.h"
#include "joints2d.h"
#include "philox.h"

namespace gator {
namespace {

constexpr int kNJ = GATOR_NOISE_COCO_JOINTS;
enum NoiseSet : uint32_t { kSetJitter = 0, kSetMiss0 = 1, kSetMiss1 = 2, kSetInv = 3, kSetGood = 4, kSetPicks = 5, kSetResample = 6, kSetStats = 7 };

// one sample's corner of the stream: the key and the counter words that do not change within it
struct Stream {
    uint64_t seed;
    uint32_t sample, step;
};

__device__ __forceinline__ Stream stream_of(uint64_t seed, int64_t step, const int64_t* step_dev, int64_t sample_offset, int b) {
    return Stream{seed, (uint32_t)(uint64_t)(sample_offset + b), (uint32_t)(uint64_t)(step_dev ? *step_dev : step)};
}

// the four words of draw site (set, joint, index)
__device__ __forceinline__ void draw(const Stream& s, uint32_t set, int joint, uint32_t index, uint32_t (&w)[4]) {
    w[0] = index; w[1] = (uint32_t)joint | set << 8; w[2] = s.sample; w[3] = s.step;
    philox_block(w, s.seed);
}

__device__ __forceinline__ double uniform_of(uint32_t w) { return ((double)w + 0.5) * 0x1p-32; }
__device__ __forceinline__ int index_of(uint32_t w, int n) { return (int)(((uint64_t)w * (uint64_t)n) >> 32); }

struct CropArgs {
    const float *joints, *detections, *rot_deg;
    const double* stats;
    const int64_t* step_dev;
    uint64_t seed;
    int64_t step, sample_offset;
    int B, J, comps, mode, res_w, res_h;
    float* crop;
    int32_t* valid;
    double* area;
};

__global__ __launch_bounds__(64) void k_noise_crop(const CropArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    __shared__ double xs_[kMaxJ * 64], ys_[kMaxJ * 64];
    const Col<double> x{xs_, (int)threadIdx.x}, y{ys_, (int)threadIdx.x};
    const int J = load_joints(a.joints + (size_t)b * a.J * a.comps, a.J, a.comps, 0, x, y);
    float* o = a.crop + (size_t)b * J * 2;
    const Box box = tight_box(x, y, J);
    float w0, h0, cx, cy;
    const bool ok = box_extent(box, w0, h0, cx, cy);
    a.valid[b] = ok ? 1 : 0;
    if (!ok) {
        for (int j = 0; j < 2 * J; ++j) o[j] = 0.f;
        if (a.area) a.area[b] = 0.0;
        return;
    }
    const Extent e = aspect_fp64(w0, h0, a.res_w, a.res_h);
    const float w = e.w, h = e.h;
    const float fx = cx - w / 2.f, fy = cy - h / 2.f;
    const double rr = M_PI * (a.rot_deg ? (double)a.rot_deg[b] : 0.0) / 180.0, sn = sin(rr), cs = cos(rr);
    double T[2][3];
    crop_affine(fx + w * 0.5f, fy + h * 0.5f, w, sn, cs, a.res_w, a.res_h, T);
    if (a.area) {
        // replace_joint_img (dataset.py:425-430): three corners of the tight float32 box through the affine, the two side lengths
        const float xmin = box.x, ymin = box.y, xmax = box.x + box.w, ymax = box.y + box.h;
        const double p1x = T[0][0] * xmin + T[0][1] * ymin + T[0][2], p1y = T[1][0] * xmin + T[1][1] * ymin + T[1][2];
        const double p2x = T[0][0] * xmax + T[0][1] * ymin + T[0][2], p2y = T[1][0] * xmax + T[1][1] * ymin + T[1][2];
        const double p3x = T[0][0] * xmax + T[0][1] * ymax + T[0][2], p3y = T[1][0] * xmax + T[1][1] * ymax + T[1][2];
        a.area[b] = sqrt((p2x - p1x) * (p2x - p1x) + (p2y - p1y) * (p2y - p1y)) * sqrt((p3x - p2x) * (p3x - p2x) + (p3y - p2y) * (p3y - p2y));
    }
    if (a.mode == GATOR_NOISE_DETECTIONS) load_joints(a.detections + (size_t)b * a.J * a.comps, a.J, a.comps, 0, x, y);
    const Stream s = stream_of(a.seed, a.step, a.step_dev, a.sample_offset, b);
    for (int j = 0; j < J; ++j) {
        float nx = (float)(T[0][0] * x[j] + T[0][1] * y[j] + T[0][2]), ny = (float)(T[1][0] * x[j] + T[1][1] * y[j] + T[1][2]);   // astype(float32)
        if (a.mode == GATOR_NOISE_STATS) {
            // generate_syn_error: float32(normal(mean, std)) per axis, kept where weight > uniform; then / 256 * [W, H] and the sum in float32
            const double* st = a.stats + (size_t)j * 5;
            uint32_t wd[4];
            draw(s, kSetStats, j, 0, wd);
            const double rad = sqrt(-2.0 * log(uniform_of(wd[0]))), ang = (2.0 * M_PI) * uniform_of(wd[1]);
            const float keep = (double)(float)st[4] > uniform_of(wd[2]) ? 1.f : 0.f;
            const float ex = (float)(st[0] + st[2] * (rad * cos(ang))) * keep, ey = (float)(st[1] + st[3] * (rad * sin(ang))) * keep;
            nx = nx + ex / 256.f * (float)a.res_w;
            ny = ny + ey / 256.f * (float)a.res_h;
        }
        o[j * 2] = nx; o[j * 2 + 1] = ny;
    }
}

// One candidate set of one joint: n points at r in [lo, hi) around (cx, cy), kept where the other centre -- if there is one -- is
// farther than `thr` (thr < 0: farther than the candidate's own r).
struct CandSet {
    uint32_t set;
    int joint, n;
    double cx, cy, ox, oy, lo, hi, thr;
    bool other;
};

// The set's accepted count when want < 0.  With want >= 0 the scan stops at the want-th accepted candidate (in candidate order) and
// leaves its coordinates in (px, py) on every lane.  Wave-uniform arguments; all 64 lanes take part.
__device__ __forceinline__ int scan_set(const Stream& s, const CandSet& c, int want, double& px, double& py) {
    const int lane = threadIdx.x;
    int count = 0;
    for (int i0 = 0; i0 < c.n; i0 += 64) {
        const int i = i0 + lane;
        uint32_t w[4];
        draw(s, c.set, c.joint, (uint32_t)i, w);
        const double angle = (2.0 * M_PI) * uniform_of(w[0]);
        const double r = c.lo + (c.hi - c.lo) * uniform_of(w[1]);
        const double x = c.cx + r * cos(angle), y = c.cy + r * sin(angle);
        bool ok = i < c.n;
        if (c.other) ok = ok && sqrt((c.ox - x) * (c.ox - x) + (c.oy - y) * (c.oy - y)) > (c.thr < 0.0 ? r : c.thr);
        const unsigned long long m = __ballot(ok);
        const int got = __popcll(m);
        if (want >= 0 && count + got > want) {
            const int k = want - count;                                              // the k-th set bit of m holds the point
            const int rank = __popcll(m & ((1ull << lane) - 1ull));
            const unsigned long long hit = __ballot(ok && rank == k);
            const int src = __ffsll((long long)hit) - 1;
            px = __shfl(x, src); py = __shfl(y, src);
            return want + 1;
        }
        count += got;
    }
    return count;
}

struct CandArgs {
    gator_coco_noise_model m;
    const float* joint_valid;
    const int32_t* valid;
    const double* area;
    const int64_t* step_dev;
    uint64_t seed;
    int64_t step, sample_offset;
    int B, J;
    float* crop;
    int32_t* decisions;
};

// synthesize_pose for joint j of a sample whose current position is (cx, cy); `other`: its partner counts as a centre, at (ox, oy).
// Returns the new position, (0, 0) when no case finds a point; dec (8 words, or null) receives the decisions.
__device__ __forceinline__ void synthesize_joint(const Stream& s, const gator_coco_noise_model& m, int j, int n_valid, double area, double cx,
                                                 double cy, bool other, double ox, double oy, float& nx, float& ny, int32_t* dec) {
    const double base = (-2.0 * area) * m.var[j];
    const double d10 = sqrt(base * m.log_ks[0]), d50 = sqrt(base * m.log_ks[1]), d85 = sqrt(base * m.log_ks[2]);
    const CandSet jitter{kSetJitter, j, m.n_jitter, cx, cy, ox, oy, d85, d50, -1.0, other};
    const CandSet miss0{kSetMiss0, j, m.n_miss, cx, cy, ox, oy, d50, d10, d50, other};
    const CandSet miss1{kSetMiss1, j, m.n_miss, ox, oy, cx, cy, d50, d10, d50, true};
    const CandSet inv{kSetInv, j, m.n_inv, ox, oy, cx, cy, 0.0, d50, -1.0, true};
    const CandSet good{kSetGood, j, m.n_good, cx, cy, ox, oy, 0.0, d85, -1.0, other};
    double px = 0.0, py = 0.0;
    const int nj = scan_set(s, jitter, -1, px, py);
    const int nm0 = scan_set(s, miss0, -1, px, py);
    const int nm1 = other ? scan_set(s, miss1, -1, px, py) : 0;
    const int ni = other ? scan_set(s, inv, -1, px, py) : 0;
    const int ng = scan_set(s, good, -1, px, py);
    const int nmiss = nm0 + nm1 / 4;                                                  // the partner's points are resampled to a quarter
    const double jp = m.jitter_prob[n_valid <= m.tier_valid[1] ? 0 : 1][j];
    const double mp = m.miss_prob[n_valid <= m.tier_valid[0] ? 0 : n_valid <= m.tier_valid[1] ? 1 : 2][j];
    const double ip = m.inv_prob[j], sp = 0.0;
    const double gp = 1.0 - (jp + mp + ip + sp);
    const double p0 = nj ? jp : 0.0, p1 = nmiss ? mp : 0.0, p2 = ni ? ip : 0.0, p4 = ng ? gp : 0.0;
    const double norm = p0 + p1 + p2 + sp + p4;
    int cs = -1, pick = -1, sub = -1;
    if (norm != 0.0) {
        // np.random.choice(5, 1, p): the cumulative sum, divided by its last entry, searched from the right for one uniform
        const double c0 = p0 / norm, c1 = c0 + p1 / norm, c2 = c1 + p2 / norm, c3 = c2 + sp / norm, c4 = c3 + p4 / norm;
        uint32_t wc[4], wp[4];
        draw(s, kSetPicks, j, 1, wc);
        draw(s, kSetPicks, j, 0, wp);
        const double u = uniform_of(wc[0]);
        cs = (c0 / c4 <= u) + (c1 / c4 <= u) + (c2 / c4 <= u) + (c3 / c4 <= u);
        if (cs == 0) {
            pick = index_of(wp[0], nj);
            scan_set(s, jitter, pick, px, py);
        } else if (cs == 1) {
            pick = index_of(wp[1], nmiss);
            if (pick < nm0) {
                scan_set(s, miss0, pick, px, py);
            } else {
                uint32_t wr[4];
                draw(s, kSetResample, j, (uint32_t)(pick - nm0), wr);
                sub = index_of(wr[0], nm1);
                scan_set(s, miss1, sub, px, py);
            }
        } else if (cs == 2) {
            pick = index_of(wp[2], ni);
            scan_set(s, inv, pick, px, py);
        } else {
            pick = index_of(wp[3], ng);
            scan_set(s, good, pick, px, py);
        }
    }
    nx = cs < 0 ? 0.f : (float)px;
    ny = cs < 0 ? 0.f : (float)py;
    if (dec && threadIdx.x == 0) {
        dec[0] = nj; dec[1] = nm0; dec[2] = nm1; dec[3] = ni; dec[4] = ng; dec[5] = cs; dec[6] = pick; dec[7] = sub;
    }
}

// grid: batch * 17 waves.  The wave of joint j works when j leads its pair (no partner, or partner > j): it perturbs j, then the
// partner with the perturbed j as its other centre.  Validity is the caller's, unchanged by the noise.
__global__ __launch_bounds__(64) void k_noise_candidates(const CandArgs a) {
    const int b = blockIdx.x / kNJ, j = blockIdx.x % kNJ;
    if (b >= a.B) return;
    const int q = a.m.partner[j];
    if ((q >= 0 && q < j) || !a.valid[b]) return;
    const float* jv = a.joint_valid ? a.joint_valid + (size_t)b * a.J : nullptr;
    int n_valid = kNJ;
    if (jv) {
        n_valid = 0;
        for (int i = 0; i < kNJ; ++i) n_valid += jv[i] > 0.f;
    }
    float* crop = a.crop + (size_t)b * a.J * 2;
    int32_t* dec = a.decisions ? a.decisions + ((size_t)b * kNJ) * 8 : nullptr;
    const Stream s = stream_of(a.seed, a.step, a.step_dev, a.sample_offset, b);
    const double area = a.area[b];
    const float jx = crop[j * 2], jy = crop[j * 2 + 1];
    float qx = 0.f, qy = 0.f;
    if (q >= 0) { qx = crop[q * 2]; qy = crop[q * 2 + 1]; }
    float nx, ny;
    synthesize_joint(s, a.m, j, n_valid, area, jx, jy, q >= 0 && (!jv || jv[q] > 0.f), qx, qy, nx, ny, dec ? dec + j * 8 : nullptr);
    float mx = 0.f, my = 0.f;
    if (q >= 0) synthesize_joint(s, a.m, q, n_valid, area, qx, qy, !jv || jv[j] > 0.f, nx, ny, mx, my, dec ? dec + q * 8 : nullptr);
    if (threadIdx.x == 0) {
        crop[j * 2] = nx; crop[j * 2 + 1] = ny;
        if (q >= 0) { crop[q * 2] = mx; crop[q * 2 + 1] = my; }
    }
}

// flip_2d_joint on the float32 joints (dataset.py:372-373, lib/aug_utils.py:33-39), /[W,H], the standardisation
__global__ __launch_bounds__(64) void k_noise_finish(const float* __restrict__ crop, const int32_t* __restrict__ valid, int B, int J,
                                                     const int32_t* __restrict__ flip, const int32_t* __restrict__ pairs, int n_pairs, int res_w,
                                                     int res_h, float* __restrict__ out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    __shared__ float fxs_[kMaxJ * 64], fys_[kMaxJ * 64];
    const Col<float> x{fxs_, (int)threadIdx.x}, y{fys_, (int)threadIdx.x};
    const float* c = crop + (size_t)b * J * 2;
    float* o = out + (size_t)b * J * 2;
    if (!valid[b]) {
        for (int j = 0; j < 2 * J; ++j) o[j] = 0.f;
        return;
    }
    for (int j = 0; j < J; ++j) { x[j] = c[j * 2]; y[j] = c[j * 2 + 1]; }
    if (flip && flip[b]) {
        for (int j = 0; j < J; ++j) x[j] = ((float)res_w - x[j]) - 1.f;
        for (int q = 0; q < n_pairs; ++q) {
            const int u = pairs[2 * q], v = pairs[2 * q + 1];
            if (u >= 0 && v >= 0 && u < J && v < J) { const float tx = x[u], ty = y[u]; x[u] = x[v]; y[u] = y[v]; x[v] = tx; y[v] = ty; }
        }
    }
    for (int j = 0; j < J; ++j) { x[j] = x[j] / (float)res_w; y[j] = y[j] / (float)res_h; }
    standardise(x, y, J, o);
}

}  // namespace
}  // namespace gator

extern "C" int gator_preprocess_noise_f32(const gator_preprocess_noise_args* args, void* stream) {
    using namespace gator;
    const char* who = "gator_preprocess_noise_f32";
    if (!args) return fail(GATOR_EINVAL, "%s: null args", who);
    GATOR_TRY(check_struct_size(who, "gator_preprocess_noise_args", args->struct_size, sizeof(gator_preprocess_noise_args)));
    const gator_preprocess_noise_args& a = *args;
    if (a.batch < 0) return fail(GATOR_EINVAL, "%s: batch %d", who, a.batch);
    if (!a.joints || !a.pose2d || !a.valid || !a.noisy_crop) return fail(GATOR_EINVAL, "%s: joints, pose2d, valid and noisy_crop are required", who);
    if (a.n_joints < 1 || a.n_joints > kMaxJ) return fail(GATOR_EINVAL, "%s: %d joints (1..%d)", who, a.n_joints, kMaxJ);
    if (a.comps < 2 || a.res_w < 1 || a.res_h < 1) return fail(GATOR_EINVAL, "%s: comps %d (>= 2), resolution %d x %d (>= 1)", who, a.comps, a.res_w, a.res_h);
    if (a.n_pairs < 0 || (a.n_pairs > 0 && !a.flip_pairs)) return fail(GATOR_EINVAL, "%s: %d flip pairs without a table", who, a.n_pairs);
    if (a.sample_offset < 0 || a.sample_offset + (int64_t)a.batch > (int64_t)1 << 32)
        return fail(GATOR_EINVAL, "%s: samples %lld .. %lld outside [0, 2^32]", who, (long long)a.sample_offset, (long long)(a.sample_offset + a.batch));
    if (a.mode == GATOR_NOISE_COCO) {
        if (a.n_joints < kNJ) return fail(GATOR_EINVAL, "%s: the coco noise needs the %d COCO joints first, got %d", who, kNJ, a.n_joints);
        if (!a.coco || !a.area) return fail(GATOR_EINVAL, "%s: the coco noise needs its model and the area output", who);
        const gator_coco_noise_model& m = *a.coco;
        for (int j = 0; j < kNJ; ++j) {
            const int q = m.partner[j];
            if (q < -1 || q >= kNJ || q == j || (q >= 0 && m.partner[q] != j))
                return fail(GATOR_EINVAL, "%s: partner[%d] = %d is no symmetric pairing of joints 0..%d", who, j, q, kNJ - 1);
        }
        for (int n : {m.n_jitter, m.n_miss, m.n_inv, m.n_good})
            if (n < 1 || n > (1 << 20)) return fail(GATOR_EINVAL, "%s: %d candidates in a set (1..2^20)", who, n);
    } else if (a.mode == GATOR_NOISE_STATS) {
        if (!a.stats) return fail(GATOR_EINVAL, "%s: the stats noise needs its [n_joints,5] table", who);
    } else if (a.mode == GATOR_NOISE_DETECTIONS) {
        if (!a.detections) return fail(GATOR_EINVAL, "%s: the detections mode needs the detections", who);
    } else {
        return fail(GATOR_EINVAL, "%s: unknown mode %d", who, a.mode);
    }
    if (a.batch == 0) return GATOR_OK;
    if ((int64_t)a.batch * kNJ > 0x7fffffffLL) return fail(GATOR_EINVAL, "%s: batch %d exceeds a grid", who, a.batch);
    hipStream_t st = (hipStream_t)stream;
    const int blocks = (a.batch + 63) / 64;
    const CropArgs ca{a.joints, a.detections, a.rot_deg, a.stats, a.step_dev, a.seed, a.step, a.sample_offset, a.batch, a.n_joints, a.comps,
                      a.mode, a.res_w, a.res_h, a.noisy_crop, a.valid, a.area};
    k_noise_crop<<<blocks, 64, 0, st>>>(ca);
    GATOR_HIP_CHECK(hipGetLastError());
    if (a.mode == GATOR_NOISE_COCO) {
        const CandArgs cd{*a.coco, a.joint_valid, a.valid, a.area, a.step_dev, a.seed, a.step, a.sample_offset, a.batch, a.n_joints, a.noisy_crop,
                          a.decisions};
        k_noise_candidates<<<a.batch * kNJ, 64, 0, st>>>(cd);
        GATOR_HIP_CHECK(hipGetLastError());
    }
    k_noise_finish<<<blocks, 64, 0, st>>>(a.noisy_crop, a.valid, a.batch, a.n_joints, a.flip, a.flip_pairs, a.n_pairs, a.res_w, a.res_h, a.pose2d);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}
