// Camera-frame training targets on the device: the deterministic part of the datasets' __getitem__ for a whole batch
// (data/Human36M/dataset.py:254-309,339-407, data/AMASS/dataset.py:182-304, PW3D / COCO / MuCo alike), around the SMPL layer:
//   gator_batch_prepare_f32  : k_batch_prepare, before the layer -- the root orientation composed with the camera rotation
//                              (Human36M:267-274, AMASS:188-196) and the mean-shape rule (Human36M:265);
//   gator_camera_targets_f32 : k_camera_targets, after the layer -- the translation into the camera frame (Human36M:287-298,
//                              AMASS:205-211), the regressed joints, cam2pixel (lib/coord_utils.py:104-109), the root-relative
//                              targets, j3d_processing (lib/aug_utils.py:67-83), the fitting-error gate (Human36M:302-309,392-401).
// The detector noise (lib/noise_utils.py) is not built here: joint_img is the pixel-space input a noise step would start from.
//
// k_batch_prepare, one lane per sample, fp64: root' = log(R exp(root)) (exp and log: so3.h).  exp is Rodrigues' formula; log goes through the quaternion
// of the product (Shepperd's choice of the largest of trace, m00, m11, m22 as the pivot), angle = 2 atan2(|q_xyz|, q_w) with q_w >= 0:
// an angle in [0, pi], accurate at both ends, where acos of the trace loses half the digits.  DEPARTURE from the reference: a zero
// root vector is the identity rotation (root' = log R); the reference divides the vector by its zero norm and produces NaN.
// A non-finite root or R gives a NaN root' for that sample; every other joint of the pose is copied bit for bit, and with R == NULL
// so is the root.  A betas row with any |beta| > 3 becomes zeros, any other row (a NaN row included) is copied bit for bit.
//
// k_camera_targets, one 256-thread workgroup per sample.  mesh_cam = (v + T) * 1000 is formed in fp64 from the float32 vertex on the
// fly; the joints are fp64 sums over the COO lists (joint j on lanes 4j .. 4j+3, partial sums added in a fixed order, as
// mesh_eval.hip's `regress`); everything after them is fp64 and each output is rounded to float32 once.  Nothing is atomic and no
// sum crosses a sample, so a sample's outputs are the same bits whatever the batch.  All reads of the vertices for the joints finish
// (a barrier) before the mesh is written, and the mesh pass reads and writes element i in the same lane: mesh == verts is allowed.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "handle.h"          // check_struct_size
#include "procrustes.h"      // wave_sum, coo_ok
#include "so3.h"             // rotvec_exp, rotmat_log

namespace gator {
namespace {

constexpr int kPrepThreads = 64;
constexpr int kCamThreads = 256, kCamMaxJoints = 64, kCamLanesPerJoint = kCamThreads / kCamMaxJoints;
constexpr double kPi = 3.141592653589793238462643383279502884;

// pose_out may be pose, betas_out may be betas: a lane reads what it needs of its own row before it writes any of it.
__global__ __launch_bounds__(kPrepThreads) void k_batch_prepare(const float* pose, const float* R, const float* betas, int B, int n_pose,
                                                                 int n_betas, int root, float* pose_out, float* betas_out) {
    const int b = blockIdx.x * kPrepThreads + threadIdx.x;
    if (b >= B) return;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(pose) + (size_t)b * n_pose;
    uint32_t* dst = reinterpret_cast<uint32_t*>(pose_out) + (size_t)b * n_pose;
    double r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = (double)pose[(size_t)b * n_pose + root * 3 + k];
    if (dst != src)
        for (int i = 0; i < n_pose; ++i) dst[i] = src[i];
    if (R) {
        double Rm[3][3], E[3][3], M[3][3], rv[3];
        bool finite = isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) { Rm[i][j] = (double)R[(size_t)b * 9 + i * 3 + j]; finite = finite && isfinite(Rm[i][j]); }
        if (finite) {
            rotvec_exp(r, E);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) M[i][j] = (Rm[i][0] * E[0][j] + Rm[i][1] * E[1][j]) + Rm[i][2] * E[2][j];
            // a float32 R is orthogonal to ~1e-7 only: one Newton step of the polar decomposition, Q = M (3 I - M^T M) / 2, is the
            // rotation nearest to M up to the square of that defect
            double G[3][3], Q[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    G[i][j] = (i == j ? 3.0 : 0.0) - ((M[0][i] * M[0][j] + M[1][i] * M[1][j]) + M[2][i] * M[2][j]);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) Q[i][j] = 0.5 * ((M[i][0] * G[0][j] + M[i][1] * G[1][j]) + M[i][2] * G[2][j]);
            rotmat_log(Q, rv);
        } else {
            rv[0] = rv[1] = rv[2] = __builtin_nan("");
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) pose_out[(size_t)b * n_pose + root * 3 + k] = (float)rv[k];
    }
    if (betas) {
        const float* bs = betas + (size_t)b * n_betas;
        float* bd = betas_out + (size_t)b * n_betas;
        bool far = false;
        for (int i = 0; i < n_betas; ++i) far = far || fabsf(bs[i]) > 3.0f;
        if (far)
            for (int i = 0; i < n_betas; ++i) bd[i] = 0.0f;
        else if (bd != bs)
            for (int i = 0; i < n_betas; ++i) reinterpret_cast<uint32_t*>(bd)[i] = reinterpret_cast<const uint32_t*>(bs)[i];
    }
}

// out[j] = (sum over the entries of row j of val * mesh_cam[col], the sum of val), fp64, mesh_cam = (v + T) * 1000.  The lane layout
// and the order of the sums are mesh_eval.hip's `regress`: entries in any order, duplicates add, a joint without entries is 0.
// The list is staged through LDS 256 entries at a time, one entry's products per lane, so that the gathers of a round are in flight
// together; a lane that scanned the list in global memory would wait for one dependent gather after another.  Lane q of a joint still
// adds entries q, q+4, ... in list order (a round starts at a multiple of 4).
__device__ void regress_cam(const gator_coo& g, const float* v, const double T[3], double (*out)[4], double (*term)[4], int* term_row) {
    const int tid = threadIdx.x, j = tid / kCamLanesPerJoint, q = tid % kCamLanesPerJoint;
    double a[4] = {0, 0, 0, 0};
    for (int base = 0; base < g.nnz; base += kCamThreads) {
        const int n = min(kCamThreads, g.nnz - base);
        __syncthreads();                                 // the previous round has been read
        if (tid < n) {
            const double w = g.val[base + tid];
            const size_t o = (size_t)g.col[base + tid] * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) term[tid][k] = w * (((double)v[o + k] + T[k]) * 1000.0);
            term[tid][3] = w;
            term_row[tid] = g.row[base + tid];
        }
        __syncthreads();
        for (int e = q; e < n; e += kCamLanesPerJoint)
            if (term_row[e] == j)
#pragma unroll
                for (int k = 0; k < 4; ++k) a[k] += term[e][k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { a[k] += __shfl_xor(a[k], 1); a[k] += __shfl_xor(a[k], 2); }
    if (q == 0 && j < g.n_joint)
#pragma unroll
        for (int k = 0; k < 4; ++k) out[j][k] = a[k];
}

__global__ __launch_bounds__(kCamThreads) void k_camera_targets(const gator_camera_targets_args a) {
    __shared__ double jh[kCamMaxJoints][4], jc[kCamMaxJoints][4];      // the regressed joints in mm, camera frame: x, y, z, sum of the row
    __shared__ double lift[kCamMaxJoints][3];                          // the lifter's target after the rotation, before the flip
    __shared__ double term[kCamThreads][4];                            // regress_cam's round: val * mesh_cam[col] and val of 256 entries
    __shared__ int term_row[kCamThreads];
    const int tid = threadIdx.x, NV = a.n_verts;
    const size_t b = blockIdx.x;
    const float* v = a.verts + b * NV * 3;
    const int Jh = a.reg_h36m.n_joint, nc = a.reg_coco.n_joint;
    const bool coco = a.lift_set == 1;
    const int Jl = coco ? nc + 2 : Jh;

    // 1. T (metres)
    double T[3];
    {
        double tr[3], ct[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { tr[k] = a.trans ? (double)a.trans[b * 3 + k] : 0.0; ct[k] = a.cam_t ? (double)a.cam_t[b * 3 + k] : 0.0; }
        if (a.compensate_root) {
            const float* Rm = a.R + b * 9;
            const float* rj = a.joints + (b * a.n_smpl_joints + a.root_idx) * 3;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double Rt = ((double)Rm[r * 3] * tr[0] + (double)Rm[r * 3 + 1] * tr[1]) + (double)Rm[r * 3 + 2] * tr[2];
                const double Rr = ((double)Rm[r * 3] * (double)rj[0] + (double)Rm[r * 3 + 1] * (double)rj[1]) + (double)Rm[r * 3 + 2] * (double)rj[2];
                T[r] = ((Rt + ct[r]) - (double)rj[r]) + Rr;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) T[k] = tr[k] + ct[k];
        }
    }

    // 2. the joints from the mesh
    regress_cam(a.reg_h36m, v, T, jh, term, term_row);
    if (coco) regress_cam(a.reg_coco, v, T, jc, term, term_row);
    __syncthreads();                                     // the last read of a vertex for the joints is behind every lane
    if (coco && tid < 3) {                               // add_pelvis_and_neck
        jc[nc][tid] = (jc[11][tid] + jc[12][tid]) * 0.5;
        jc[nc + 1][tid] = (jc[5][tid] + jc[6][tid]) * 0.5;
    }
    const float* dc = a.joint_cam ? a.joint_cam + b * Jh * 3 : nullptr;
    double rh[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) rh[k] = dc ? (double)dc[k] : jh[0][k];

    // 5. the mesh: element i is read and written by the same lane
    float* m = a.mesh + b * NV * 3;
    for (int i = tid; i < NV * 3; i += kCamThreads) {
        const int k = i % 3;
        m[i] = (float)(((((double)v[i] + T[k]) * 1000.0) - rh[k]) / 1000.0);
    }
    __syncthreads();                                     // pelvis and neck

    // 4. / 5. the joints: lane j has joint j of each set
    double reg[3] = {0, 0, 0};
    if (tid < Jh) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            reg[k] = dc ? (double)dc[tid * 3 + k] - (double)dc[k] : jh[tid][k] - jh[0][k];
            a.reg_pose3d[(b * Jh + tid) * 3 + k] = (float)reg[k];
        }
    }
    if (tid < Jl) {
        double p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = coco ? jc[tid][k] - jc[nc][k] : reg[k];
        const float r = a.rot_deg ? a.rot_deg[b] : 0.0f;
        if (r != 0.0f) {                                 // j3d_processing: about z by -rot_deg
            const double rad = -(double)r * kPi / 180.0;
            const double sn = sin(rad), cs = cos(rad);
            const double x = cs * p[0] - sn * p[1], y = sn * p[0] + cs * p[1];
            p[0] = x; p[1] = y;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) lift[tid][k] = p[k];
    }
    __syncthreads();
    if (tid < Jl) {
        const bool fl = a.flip && a.flip[b] != 0;
        int src = tid;
        if (fl)                                          // flip_3d_joint swaps pair after pair: walk the list backwards to the source
            for (int e = a.n_pairs - 1; e >= 0; --e) {
                const int u = a.flip_pairs[2 * e], w = a.flip_pairs[2 * e + 1];
                if (u < 0 || w < 0 || u >= Jl || w >= Jl) continue;
                if (src == u) src = w; else if (src == w) src = u;
            }
        float* lo = a.lift_pose3d + (b * Jl + tid) * 3;
        lo[0] = (float)(fl ? -lift[src][0] : lift[src][0]);
        lo[1] = (float)lift[src][1];
        lo[2] = (float)lift[src][2];
        // 3. cam2pixel
        float* ji = a.joint_img_out + (b * Jl + tid) * 2;
        if (!coco && a.joint_img) {
            ji[0] = a.joint_img[(b * Jh + tid) * 2];
            ji[1] = a.joint_img[(b * Jh + tid) * 2 + 1];
        } else {
            const double* P = coco ? jc[tid] : jh[tid];
            ji[0] = (float)(P[0] / P[2] * (double)a.focal[b * 2] + (double)a.princpt[b * 2]);
            ji[1] = (float)(P[1] / P[2] * (double)a.focal[b * 2 + 1] + (double)a.princpt[b * 2 + 1]);
        }
    }

    // get_fitting_error and the masks: the first wave, lane j with joint j
    if (tid < 64) {
        double err = __builtin_nan("");
        if (dc) {
            const bool on = tid < Jh;
            double h[3] = {0, 0, 0}, f[3] = {0, 0, 0}, mh[3], mf[3];
            if (on)
#pragma unroll
                for (int k = 0; k < 3; ++k) { h[k] = reg[k]; f[k] = jh[tid][k] - jh[tid][3] * rh[k]; }      // J (mesh_cam - root), row by row
#pragma unroll
            for (int k = 0; k < 3; ++k) { mh[k] = wave_sum(h[k]) / Jh; mf[k] = wave_sum(f[k]) / Jh; }
            double d2 = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double d = h[k] - ((f[k] - mf[k]) + mh[k]); d2 += d * d; }
            err = wave_sum(on ? sqrt(d2) : 0.0) / Jh;
        }
        if (tid == 0) {
            const bool far = dc && err > (double)a.fitting_thr;
            a.fit_error[b] = (float)err;
            a.valid[b * 3] = far ? 0.0f : 1.0f;
            a.valid[b * 3 + 1] = far && coco ? 0.0f : 1.0f;
            a.valid[b * 3 + 2] = 1.0f;
        }
    }
}

}  // namespace
}  // namespace gator

extern "C" int gator_batch_prepare_f32(const float* pose, const float* R, const float* betas, int32_t batch, int32_t n_pose, int32_t n_betas,
                                       int32_t root_idx, float* pose_out, float* betas_out, void* stream) {
    using namespace gator;
    const char* who = "gator_batch_prepare_f32";
    if (batch < 0) return fail(GATOR_EINVAL, "%s: batch %d", who, batch);
    if (n_pose < 3 || n_pose % 3 != 0) return fail(GATOR_EINVAL, "%s: n_pose %d (three per joint, at least one joint)", who, n_pose);
    if (root_idx < 0 || root_idx >= n_pose / 3) return fail(GATOR_EINVAL, "%s: root_idx %d outside [0, %d)", who, root_idx, n_pose / 3);
    if (betas && n_betas < 1) return fail(GATOR_EINVAL, "%s: betas with n_betas %d", who, n_betas);
    if (batch == 0) return GATOR_OK;
    if (!pose || !pose_out) return fail(GATOR_EINVAL, "%s: null pose or pose_out", who);
    if (betas && !betas_out) return fail(GATOR_EINVAL, "%s: betas without betas_out", who);
    k_batch_prepare<<<(batch + kPrepThreads - 1) / kPrepThreads, kPrepThreads, 0, (hipStream_t)stream>>>(pose, R, betas, batch, n_pose, n_betas,
                                                                                                      root_idx, pose_out, betas_out);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

extern "C" int gator_camera_targets_f32(const gator_camera_targets_args* args, void* stream) {
    using namespace gator;
    const char* who = "gator_camera_targets_f32";
    if (!args) return fail(GATOR_EINVAL, "%s: null args", who);
    GATOR_TRY(check_struct_size(who, "gator_camera_targets_args", args->struct_size, sizeof(gator_camera_targets_args)));
    const gator_camera_targets_args& a = *args;
    if (a.batch < 0) return fail(GATOR_EINVAL, "%s: batch %d", who, a.batch);
    if (a.n_verts < 1) return fail(GATOR_EINVAL, "%s: n_verts %d (at least 1)", who, a.n_verts);
    if (a.n_smpl_joints < 1 || a.root_idx < 0 || a.root_idx >= a.n_smpl_joints)
        return fail(GATOR_EINVAL, "%s: root_idx %d outside [0, %d)", who, a.root_idx, a.n_smpl_joints);
    if (a.lift_set != GATOR_LIFT_HUMAN36 && a.lift_set != GATOR_LIFT_COCO) return fail(GATOR_EINVAL, "%s: lift_set %d (0 human36, 1 coco)", who, a.lift_set);
    if (!coo_ok(a.reg_h36m) || a.reg_h36m.n_joint < 1 || a.reg_h36m.n_joint > kCamMaxJoints)
        return fail(GATOR_EINVAL, "%s: reg_h36m (nnz >= 0 with its arrays, 1..%d joints)", who, kCamMaxJoints);
    if (a.reg_h36m_n_verts != a.n_verts)
        return fail(GATOR_EINVAL, "%s: reg_h36m over %d vertices, meshes of %d", who, a.reg_h36m_n_verts, a.n_verts);
    const bool has_coco = a.reg_coco.n_joint != 0;
    if (a.lift_set == GATOR_LIFT_COCO && !has_coco) return fail(GATOR_EINVAL, "%s: lift_set coco without reg_coco", who);
    if (has_coco) {
        if (!coo_ok(a.reg_coco) || a.reg_coco.n_joint < 13 || a.reg_coco.n_joint > kCamMaxJoints - 2)
            return fail(GATOR_EINVAL, "%s: reg_coco (nnz >= 0 with its arrays, 13..%d joints: pelvis and neck come from joints 5, 6, 11, 12)", who,
                        kCamMaxJoints - 2);
        if (a.reg_coco_n_verts != a.n_verts)
            return fail(GATOR_EINVAL, "%s: reg_coco over %d vertices, meshes of %d", who, a.reg_coco_n_verts, a.n_verts);
    }
    if (a.compensate_root && !a.R) return fail(GATOR_EINVAL, "%s: compensate_root without R", who);
    if (a.joint_cam && !a.joint_img && a.lift_set == GATOR_LIFT_HUMAN36)
        return fail(GATOR_EINVAL, "%s: the dataset's joint_cam without its joint_img for the human36 lift set", who);
    if (a.n_pairs < 0 || (a.n_pairs > 0 && !a.flip_pairs)) return fail(GATOR_EINVAL, "%s: n_pairs %d with%s flip_pairs", who, a.n_pairs, a.flip_pairs ? "" : "out");
    if (a.batch == 0) return GATOR_OK;
    if (!a.verts || !a.focal || !a.princpt || (a.compensate_root && !a.joints))
        return fail(GATOR_EINVAL, "%s: null verts, focal, princpt or (with compensate_root) joints", who);
    if (!a.mesh || !a.reg_pose3d || !a.lift_pose3d || !a.joint_img_out || !a.fit_error || !a.valid) return fail(GATOR_EINVAL, "%s: null output", who);
    k_camera_targets<<<a.batch, kCamThreads, 0, (hipStream_t)stream>>>(a);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}
