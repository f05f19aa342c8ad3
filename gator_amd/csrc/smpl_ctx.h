// The SMPL handle (gator_smpl_*): the packed model and the workspaces of its three users, the layer (smpl_lbs.hip), the fit
// (smpl_fit.hip) and the layer's backward (smpl_backward.hip), with the host steps their entries share.  The device steps they share
// are in smpl_steps.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "handle.h"

namespace gator {
constexpr int kSmplMaxJ = 32, kSmplMaxB = 16;
constexpr int kTV = 128;     // vertices per tile of the layer: four waves of 32 columns; the vertex planes are padded to whole tiles
}  // namespace gator

struct gator_smpl : gator::Handle {
    int NV = 0, NJ = 0, NB = 0, K = 0, Kp = 0, NVp = 0, MI = 0;
    gator::DevBuf<float> basis;      // [3][Kp][NVp]  coordinate planes of [shapedirs | posedirs], zero padded
    gator::DevBuf<float> vtempl;     // [3][NVp]
    gator::DevBuf<int32_t> widx;     // [MI][NVp]     skinning influences of a vertex: joint index ...
    gator::DevBuf<float> wval;       // [MI][NVp]     ... and weight (0 in unused slots)
    gator::DevBuf<double> jfold;     // [NJ*3][1+NB]  J_regressor . v_template, J_regressor . shapedirs (folded in fp64)
    gator::DevBuf<int32_t> parents;  // [NJ]
    // workspace of the forward, grown when a larger batch arrives (gator::Handle::grow per buffer; cap is the batch all three hold)
    gator::WorkBuf<float> coef;      // [cap][Kp]
    gator::WorkBuf<float> xform;     // [cap][NJ][12]
    gator::WorkBuf<float> offs;      // [cap][4]
    int cap = 0;
    // the fit: model side (folded at create), then its workspace, grown like the forward's
    gator::DevBuf<uint32_t> amask;   // [MI][NVp]     bit k: joint k is the influence's joint or one of its ancestors (MI <= 4 only)
    double tcen[3] = {0, 0, 0};      // centroid of v_template
    gator::WorkBuf<float> fjoints;   // [fcap][NJ][3] posed joints of the candidate
    gator::WorkBuf<float> fstate;    // [2][fcap][P]  candidate, current: pose | betas | trans, three arrays each
    gator::WorkBuf<double> fscal;    // [fcap][4]     lambda, squared error of the current state, bad-sample flag
    gator::WorkBuf<float> fpart;     // [fcap][S][pairs][32][32] per-chunk partial sums of M's upper tiles
    gator::WorkBuf<float> fM;        // [2][fcap][N][N] M of the candidate, of the current state
    int fcap = 0;
    // the backward (smpl_backward.hip): the basis once more, coefficient-minor, then its workspace, each block grown on its own
    int Kq = 0;                      // Kp rounded up to whole 32-coefficient MFMA tiles
    gator::WorkBuf<float> basisT;    // [3][NVp][Kq]  [shapedirs | posedirs] transposed, zero padded; made by the first backward with grad_verts
    gator::WorkBuf<float> bpart;     // [sample tiles][NVp / kTV][Kq + 12 NJ][32] per-vertex-tile partial sums of g_coef and gA
    gator::WorkBuf<double> btrans;   // [sample tiles][NVp / kTV][3][32]          ... of sum_v gx
    gator::WorkBuf<double> bsum;     // [batch][Kq + 12 NJ + 4]                    their sums over the vertex tiles
};

namespace gator {
// The layer's Rodrigues (rodrigues_layer.py:13-52) in fp64: angle = |axisang + 1e-8|, quaternion (cos, sin . axisang / angle), normalised
// (axisang / angle is no unit vector), then quat2mat.  r: 3x3 row-major.
__device__ inline void smpl_rodrigues(double ax, double ay, double az, double* r) {
    const double ex = ax + 1e-8, ey = ay + 1e-8, ez = az + 1e-8;             // batch_rodrigues: norm(axisang + 1e-8)
    const double angle = sqrt(ex * ex + ey * ey + ez * ez);
    const double half = angle * 0.5, sn = sin(half);
    double w = cos(half), x = sn * (ax / angle), y = sn * (ay / angle), z = sn * (az / angle);
    const double qn = sqrt(w * w + x * x + y * y + z * z);                   // quat2mat normalises: axisang / angle is no unit vector
    w /= qn; x /= qn; y /= qn; z /= qn;
    const double w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z, wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
    r[0] = w2 + x2 - y2 - z2; r[1] = 2 * xy - 2 * wz;    r[2] = 2 * wy + 2 * xz;
    r[3] = 2 * wz + 2 * xy;   r[4] = w2 - x2 + y2 - z2;  r[5] = 2 * yz - 2 * wx;
    r[6] = 2 * xz - 2 * wy;   r[7] = 2 * wx + 2 * yz;    r[8] = w2 - x2 - y2 + z2;
}

// What every batched entry checks first: there is a ctx on the current device, and batch lies in 0 .. max_batch.
int smpl_check_batch(const char* who, const gator_smpl* ctx, int batch, int max_batch);
// The arguments the forward and the backward share: center_idx only without trans, smpl_check_batch up to 65535 sample tiles, a pose
// for a batch that is not empty, center_idx below the joint count, a finite out_scale.
int smpl_check_layer_call(const char* who, const gator_smpl* ctx, const float* pose, const float* trans, int batch, int center_idx,
                          float out_scale);

// One launch of a kernel pair by the model's influences per vertex: the MI_T = 4 form holds at most four in registers (SMPL, MANO),
// the MI_T = 0 form reads any number from the lists.  256 threads.
template <class... P, class... A>
int launch_by_influences(const gator_smpl* c, void (*k4)(P...), void (*k0)(P...), dim3 grid, size_t lds, hipStream_t st, const A&... args) {
    (c->MI <= 4 ? k4 : k0)<<<grid, 256, lds, st>>>(args...);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

int smpl_reserve(gator_smpl* c, int B);                                  // the forward's workspace for a batch of B
// k_smpl_pose on the ctx's workspace (coefficient rows, skinning transforms, offsets); center < 0: no centring
int smpl_pose_stage(gator_smpl* c, const float* pose, const float* betas, const float* trans, int batch, int center, double out_scale,
                    float* joints, hipStream_t st);
int smpl_fit_build(gator_smpl* c, const gator_smpl_model* m);            // smpl_fit.hip: the fit's share of gator_smpl_create
int smpl_backward_build(gator_smpl* c, const gator_smpl_model* m);       // smpl_backward.hip: the backward's share
}  // namespace gator
