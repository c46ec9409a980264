// k_metrics.hip -- pose-error metrics of the evaluation on the device: ADD and ADD-S (BOP "adi") of F pose pairs over one point
// set, in double precision (tools/third_party/bop_pose_error.py:73-108; the brute-force form is oracle/ro_metrics.c).
//
//   ADD[f]   = mean_i | (R_e p_i + t_e) - (R_r p_i + t_r) |
//   ADD-S[f] = mean_i min_j | (R_r p_i + t_r) - (R_e p_j + t_e) |        (ground truth -> estimate)
//
// Shape.  Both clouds are compared in the camera frame, as the oracle does, so that a quaternion is used exactly as it is given
// (a non-unit quaternion gives a matrix that is not a rotation; moving the queries into the estimate's object frame instead
// would silently assume that it is one).
//   pose_cloud_kernel   ADD-S only: the estimated cloud R_e p_j + t_e of every pose of a launch, once, into scratch memory
//                       (rows padded to a multiple of kCandBatch with copies of the last point: a duplicate changes no minimum).
//   pose_error_kernel   one workgroup of 4 waves per (pose, 1024 query points).  A lane transforms its <= 4 query points once and
//                       keeps them and their running minimum SQUARED distance in registers.  The candidates are the same for
//                       every lane of a wave: they are read with uniform (scalar) loads, kCandBatch at a time, and enter the
//                       VALU as scalar operands -- no LDS, no barrier.  Per pair: 3 sub, 1 mul, 2 fma, 1 min = 7 fp64 VALU
//                       operations (9 with ROFT_POSE_ERRORS_FMA=0: the oracle's own operation order).  One square root per
//                       query at the end, a shuffle-tree sum over the wave, one partial sum per wave with an ordinary store.
//   pose_error_finish_kernel   adds the partial sums of a pose in index order and divides by the number of points.
// Determinism: which lane holds which query, the order of the candidates and the order of every sum depend on the number of
// points only -- out[f] is a function of (kind, points, est[f], ref[f]) and of nothing else (no atomics, no dependence on the grid).
// A non-finite pose: every distance is NaN or inf, fmin keeps the running minimum at +inf, the pose's result is inf or NaN.
//
// The poses are read through PoseView: rows of 7 doubles (x y z, q = w x y z) at a stride, optionally in a ring -- the host
// arrays of roft_pose_errors and the records of the engine's log (roft_engine_score_log) go through the same kernels.
//
// MSSD and MSPD of the same pose pairs under a symmetry group have a kernel of their own further down (pose_error_sym_kernel).
#include "roft_device.h"
#include "symmetry.h"

namespace roft {

constexpr int kPoseWaves = 4;              // waves per workgroup
constexpr int kPoseSlots = 4;              // query points per lane
constexpr int kQueriesPerWave = 64 * kPoseSlots;
constexpr int kQueriesPerGroup = kPoseWaves * kQueriesPerWave;

struct RigidPose {
    double R[9], t[3];
};

// metrics.quat_to_rot, operation by operation (the file is built with -ffp-contract=off)
__device__ inline RigidPose load_pose(const PoseView& v, int f)
{
    const long row = v.ring > 0 ? (long)((v.first + f) % v.ring) : (long)(v.first + f);
    const double* p = v.base + row * v.stride;
    const double w = p[3], x = p[4], y = p[5], z = p[6];
    RigidPose g;
    g.R[0] = 1.0 - 2.0 * (y * y + z * z); g.R[1] = 2.0 * (x * y - w * z);       g.R[2] = 2.0 * (x * z + w * y);
    g.R[3] = 2.0 * (x * y + w * z);       g.R[4] = 1.0 - 2.0 * (x * x + z * z); g.R[5] = 2.0 * (y * z - w * x);
    g.R[6] = 2.0 * (x * z - w * y);       g.R[7] = 2.0 * (y * z + w * x);       g.R[8] = 1.0 - 2.0 * (x * x + y * y);
    g.t[0] = p[0]; g.t[1] = p[1]; g.t[2] = p[2];
    return g;
}

// ro_metrics.c transform(): R[i][0] p0 + R[i][1] p1 + R[i][2] p2 + t[i], left to right
__device__ inline void pose_transform(const RigidPose& g, const double* p, double o[3])
{
    for (int i = 0; i < 3; ++i) o[i] = g.R[i * 3] * p[0] + g.R[i * 3 + 1] * p[1] + g.R[i * 3 + 2] * p[2] + g.t[i];
}

__global__ __launch_bounds__(256) void pose_cloud_kernel(const double* __restrict__ pts, int P, int P_pad, PoseView est, int f0,
                                                         double* __restrict__ cloud)
{
    const int f = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= P_pad) return;
    const RigidPose g = load_pose(est, f0 + f);
    double o[3];
    pose_transform(g, pts + 3 * (size_t)min(j, P - 1), o);
    double* c = cloud + ((size_t)f * P_pad + j) * 3;
    c[0] = o[0]; c[1] = o[1]; c[2] = o[2];
}

// the nearest-neighbour search of one wave: NQ query points per lane against the P_pad candidates of the pose.  Returns the lane's
// sum of nearest distances; last_valid: the lane's last slot holds a point (only the last slot of a wave can be partly filled)
template <int NQ, bool FMA>
__device__ inline double nearest_sum(const double (&q)[kPoseSlots][3], bool last_valid, const double* __restrict__ cand, int P_pad)
{
    double best[NQ];
    for (int s = 0; s < NQ; ++s) best[s] = INFINITY;
    for (int j = 0; j < P_pad; j += kCandBatch) {
        const double* c = cand + 3 * (size_t)j;   // uniform over the wave: scalar loads
#pragma unroll
        for (int k = 0; k < kCandBatch; ++k) {
            const double ex = c[3 * k], ey = c[3 * k + 1], ez = c[3 * k + 2];
#pragma unroll
            for (int s = 0; s < NQ; ++s) {
                const double dx = ex - q[s][0], dy = ey - q[s][1], dz = ez - q[s][2];
                const double d = FMA ? __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx)) : dx * dx + dy * dy + dz * dz;
                best[s] = __builtin_fmin(best[s], d);
            }
        }
    }
    double sum = 0.0;
    for (int s = 0; s < NQ - 1; ++s) sum += sqrt(best[s]);
    const double d = sqrt(best[NQ - 1]);
    return sum + (last_valid ? d : 0.0);
}

// grid (ceil(P / 1024), poses of the launch): pose f0 + blockIdx.y, partial[blockIdx.y][wave of the pose]
template <int KIND, bool FMA>
__global__ __launch_bounds__(64 * kPoseWaves) void pose_error_kernel(const double* __restrict__ pts, int P, int P_pad, PoseView est, PoseView ref,
                                                                 int f0, const double* __restrict__ cloud, double* __restrict__ partial,
                                                                 int waves_per_pose)
{
    const int f = blockIdx.y;
    const int wave = blockIdx.x * kPoseWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int q0 = wave * kQueriesPerWave;   // slot s of lane l: point q0 + 64 s + l
    if (q0 >= P) return;                     // (wave-uniform)
    // a wave of the last group of a pose may hold fewer than kPoseSlots x 64 points: it works on the slots it has
    const int nq = min(kPoseSlots, (P - q0 + 63) >> 6);
    const bool last_valid = q0 + 64 * (nq - 1) + lane < P;
    const RigidPose gr = load_pose(ref, f0 + f);
    double q[kPoseSlots][3];
    for (int s = 0; s < kPoseSlots; ++s) pose_transform(gr, pts + 3 * (size_t)min(q0 + 64 * s + lane, P - 1), q[s]);
    double sum = 0.0;
    if (KIND == ROFT_POSE_ERROR_ADD) {
        const RigidPose ge = load_pose(est, f0 + f);
        for (int s = 0; s < kPoseSlots; ++s) {
            const int i = q0 + 64 * s + lane;
            double a[3];
            pose_transform(ge, pts + 3 * (size_t)min(i, P - 1), a);
            const double dx = a[0] - q[s][0], dy = a[1] - q[s][1], dz = a[2] - q[s][2];
            const double d = sqrt(dx * dx + dy * dy + dz * dz);   // ro_add's order
            sum += i < P ? d : 0.0;
        }
    } else {
        const double* cand = cloud + (size_t)f * P_pad * 3;
        if (nq == 4) sum = nearest_sum<4, FMA>(q, last_valid, cand, P_pad);
        else if (nq == 3) sum = nearest_sum<3, FMA>(q, last_valid, cand, P_pad);
        else if (nq == 2) sum = nearest_sum<2, FMA>(q, last_valid, cand, P_pad);
        else sum = nearest_sum<1, FMA>(q, last_valid, cand, P_pad);
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) partial[(size_t)f * waves_per_pose + wave] = sum;
}

// one thread per pose: the partial sums in index order
__global__ __launch_bounds__(256) void pose_error_finish_kernel(const double* __restrict__ partial, int waves_per_pose, int P, int n,
                                                                double* __restrict__ out)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
    double s = 0.0;
    for (int w = 0; w < waves_per_pose; ++w) s += partial[(size_t)f * waves_per_pose + w];
    out[f] = s / (double)P;
}

// ---- MSSD / MSPD (BOP: maximum symmetry-aware surface / projection distance; include/roft_engine.h section 3h) --------------------
//   p' = R_g p_i + t_g,  a = R_r p' + t_r,  b = R_e p_i + t_e                       (pose_transform's order, load_pose's matrices)
//   MSSD[f] = sqrt( min_g max_i |b - a|^2 ),   MSPD[f] = the same over the pixels (fx X / Z + cx, fy Y / Z + cy) of a and b
// One workgroup of 4 waves per pose pair.  kSymBatch elements at a time: their transforms are the same for every lane (uniform
// loads), a lane walks the points tid, tid + 256, ... once per batch and keeps one running maximum per element of the batch in
// registers; a shuffle tree gives the maximum of a wave, the LDS that of the workgroup, and every thread folds the batch into its
// running minimum.  A batch that the group does not fill repeats the last element (a duplicate changes no minimum).
// Max and min are exact and keep a NaN once they have seen one (nan_max / nan_min: fmax would drop it), so out[f] is a function
// of (kind, points, group, camera, pose pair f) and of nothing else, and a non-finite pose gives a non-finite result.
// MSPD: a point with Z <= 0 (or NaN) under either pose, for any element, makes the pair's result +inf.
constexpr int kSymBatch = 4;
constexpr int kSymThreads = 64 * kPoseWaves;

__device__ inline double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }
__device__ inline double nan_min(double a, double b) { return (b < a || b != b) ? b : a; }

template <int KIND>
__global__ __launch_bounds__(kSymThreads) void pose_error_sym_kernel(const double* __restrict__ pts, int P, PoseView est, PoseView ref, int f0,
                                                                     const double* __restrict__ elems, int n_sym, SymCamera cam,
                                                                     double* __restrict__ out)
{
    __shared__ double s_max[kPoseWaves][kSymBatch];
    const int f = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const RigidPose ge = load_pose(est, f0 + f), gr = load_pose(ref, f0 + f);
    double best = INFINITY;
    int bad = 0;
    for (int g0 = 0; g0 < n_sym; g0 += kSymBatch) {
        RigidPose gs[kSymBatch];
#pragma unroll
        for (int k = 0; k < kSymBatch; ++k) {
            const double* el = elems + sym::kElement * min(g0 + k, n_sym - 1);   // uniform over the workgroup
            sym::quat_to_rot(el[3], el[4], el[5], el[6], gs[k].R);
            gs[k].t[0] = el[0]; gs[k].t[1] = el[1]; gs[k].t[2] = el[2];
        }
        double m[kSymBatch];
#pragma unroll
        for (int k = 0; k < kSymBatch; ++k) m[k] = 0.0;
        for (int i = tid; i < P; i += kSymThreads) {
            const double* p = pts + 3 * (size_t)i;
            double b[3], ub = 0.0, vb = 0.0;
            pose_transform(ge, p, b);
            if (KIND == ROFT_POSE_ERROR_MSPD) {
                bad |= !(b[2] > 0.0);
                ub = cam.fx * b[0] / b[2] + cam.cx;
                vb = cam.fy * b[1] / b[2] + cam.cy;
            }
#pragma unroll
            for (int k = 0; k < kSymBatch; ++k) {
                double ps[3], a[3], d;
                pose_transform(gs[k], p, ps);
                pose_transform(gr, ps, a);
                if (KIND == ROFT_POSE_ERROR_MSPD) {
                    bad |= !(a[2] > 0.0);
                    const double du = ub - (cam.fx * a[0] / a[2] + cam.cx), dv = vb - (cam.fy * a[1] / a[2] + cam.cy);
                    d = du * du + dv * dv;
                } else {
                    const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
                    d = dx * dx + dy * dy + dz * dz;
                }
                m[k] = nan_max(m[k], d);
            }
        }
#pragma unroll
        for (int k = 0; k < kSymBatch; ++k) {
            for (int o = 32; o > 0; o >>= 1) m[k] = nan_max(m[k], __shfl_xor(m[k], o, 64));
            if (lane == 0) s_max[wave][k] = m[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kSymBatch; ++k) {
            double v = s_max[0][k];
            for (int w = 1; w < kPoseWaves; ++w) v = nan_max(v, s_max[w][k]);
            best = nan_min(best, v);
        }
        __syncthreads();   // (the next batch overwrites s_max)
    }
    if (KIND == ROFT_POSE_ERROR_MSPD) bad = __syncthreads_or(bad);
    if (tid == 0) out[f0 + f] = bad ? INFINITY : sqrt(best);
}

void launch_pose_errors_sym(int kind, const double* pts, int P, const PoseView& est, const PoseView& ref, int f0, int n, const double* elems,
                            int n_sym, const SymCamera& cam, double* out, hipStream_t s)
{
    if (kind == ROFT_POSE_ERROR_MSPD)
        hipLaunchKernelGGL((pose_error_sym_kernel<ROFT_POSE_ERROR_MSPD>), dim3(n), dim3(kSymThreads), 0, s, pts, P, est, ref, f0, elems, n_sym, cam, out);
    else
        hipLaunchKernelGGL((pose_error_sym_kernel<ROFT_POSE_ERROR_MSSD>), dim3(n), dim3(kSymThreads), 0, s, pts, P, est, ref, f0, elems, n_sym, cam, out);
}

__global__ __launch_bounds__(256) void float_to_double_kernel(const float* __restrict__ in, int n, double* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}

int pose_error_padded_points(int P) { return (P + kCandBatch - 1) / kCandBatch * kCandBatch; }
int pose_error_waves(int P) { return (P + kQueriesPerWave - 1) / kQueriesPerWave; }

void launch_float_to_double(const float* in, int n, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(float_to_double_kernel, dim3((n + 255) / 256), dim3(256), 0, s, in, n, out);
}

void launch_pose_errors(int kind, const double* pts, int P, const PoseView& est, const PoseView& ref, int f0, int n, double* cloud,
                        double* partial, double* out, bool fma, hipStream_t s)
{
    const int P_pad = pose_error_padded_points(P), waves = pose_error_waves(P);
    const dim3 grid((P + kQueriesPerGroup - 1) / kQueriesPerGroup, n), block(64 * kPoseWaves);
    if (kind == ROFT_POSE_ERROR_ADD) {
        hipLaunchKernelGGL((pose_error_kernel<ROFT_POSE_ERROR_ADD, false>), grid, block, 0, s, pts, P, P_pad, est, ref, f0, cloud, partial, waves);
    } else {
        hipLaunchKernelGGL(pose_cloud_kernel, dim3((P_pad + 255) / 256, n), dim3(256), 0, s, pts, P, P_pad, est, f0, cloud);
        if (fma)
            hipLaunchKernelGGL((pose_error_kernel<ROFT_POSE_ERROR_ADDS, true>), grid, block, 0, s, pts, P, P_pad, est, ref, f0, cloud, partial, waves);
        else
            hipLaunchKernelGGL((pose_error_kernel<ROFT_POSE_ERROR_ADDS, false>), grid, block, 0, s, pts, P, P_pad, est, ref, f0, cloud, partial, waves);
    }
    hipLaunchKernelGGL(pose_error_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, s, partial, waves, P, n, out + f0);
}

}  // namespace roft
