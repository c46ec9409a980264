// Probe: what a 12 x 12 Cholesky factorisation with the row in registers (k_ukf.hip, cholesky_rows) is made of, one wave alone.
//   variant 0: the plain right-looking form (all updates of a column, then the next pivot)
//   variant 1: software-pipelined by hand (next pivot from lane J + 1's own l, the updates of column J - 1 one per chain step of column J)
//   variant 2: the dependency chain ONLY (pivot broadcast -> v_rsq_f64 -> two Newton steps -> scale -> next pivot; no updates: wrong factor)
//   variant 3: the 66 updates ONLY (two DPP moves + one FMA each; no reciprocal square roots: wrong factor)
// Shader cycles, best of six, including the LDS row loads / stores and one barrier.  Build: hipcc --offload-arch=gfx950 -O3 -std=c++17
// MI355X: 2904 / 2964 / 2120 / 2100 -- the chain alone and the updates alone each cost what 70 % of the whole costs, the two already
// overlap, and pipelining by hand moves nothing (docs/notebook.md, round 7).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>
template <int SRC> __device__ __forceinline__ double rowbcast_f64(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), 0x150 + SRC, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), 0x150 + SRC, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
#define SB() __builtin_amdgcn_sched_barrier(0)
// ---- Cholesky variants -------------------------------------------------------------------------
__device__ __forceinline__ double fast_rsqrt(double d)
{
    double y = __builtin_amdgcn_rsq(d);
    const double h = 0.5 * d;
    y = fma(y, fma(-h * y, y, 0.5), y);
    y = fma(y, fma(-h * y, y, 0.5), y);
    return y;
}
namespace v0 {
template <int M, int J, int K> __device__ __forceinline__ void chol_update(double (&a)[M], double lij)
{
    if constexpr (K < M) { a[K] = fma(-lij, rowbcast_f64<K>(lij), a[K]); chol_update<M, J, K + 1>(a, lij); }
}
template <int M, int J> __device__ __forceinline__ void chol_columns(double (&a)[M], double (&rinv)[M], int& ok, int lane)
{
    if constexpr (J < M) {
        const double d = rowbcast_f64<J>(a[J]);
        if (!(d > 0.0)) ok = 0;
        const double r = fast_rsqrt(d);
        rinv[J] = r;
        const double lij = (lane == J) ? d * r : a[J] * r;
        a[J] = lij;
        chol_update<M, J, J + 1>(a, lij);
        chol_columns<M, J + 1>(a, rinv, ok, lane);
    }
}
}
namespace v1 {
template <int M, int JP, int K> __device__ __forceinline__ void chol_shadow(double (&a)[M], double lprev)
{
    if constexpr (JP >= 0 && K < M) a[K] = fma(-lprev, rowbcast_f64<K>(lprev), a[K]);
    SB();
}
template <int M, int J> __device__ __forceinline__ void chol_columns(double (&a)[M], double (&rinv)[M], int& ok, int lane, double dloc, double lprev)
{
    if constexpr (J < M) {
        constexpr int JP = J - 1;
        const double d = rowbcast_f64<J>(dloc);
        chol_shadow<M, JP, J>(a, lprev);
        if (!(d > 0.0)) ok = 0;
        const double num = (lane == J) ? d : a[J];
        double y = __builtin_amdgcn_rsq(d);
        const double h = 0.5 * d;
        chol_shadow<M, JP, J + 1>(a, lprev);
        double t = -h * y;
        chol_shadow<M, JP, J + 2>(a, lprev);
        double u = fma(t, y, 0.5);
        chol_shadow<M, JP, J + 3>(a, lprev);
        y = fma(y, u, y);
        chol_shadow<M, JP, J + 4>(a, lprev);
        t = -h * y;
        chol_shadow<M, JP, J + 5>(a, lprev);
        u = fma(t, y, 0.5);
        chol_shadow<M, JP, J + 6>(a, lprev);
        y = fma(y, u, y);
        chol_shadow<M, JP, J + 7>(a, lprev);
        rinv[J] = y;
        const double lij = num * y;
        a[J] = lij;
        chol_shadow<M, JP, J + 8>(a, lprev);
        double dnext = 0.0;
        if constexpr (J + 1 < M) dnext = fma(-lij, lij, a[J + 1]);
        chol_shadow<M, JP, J + 9>(a, lprev);
        chol_shadow<M, JP, J + 10>(a, lprev);
        chol_columns<M, J + 1>(a, rinv, ok, lane, dnext, lij);
    }
}
}
// v2: chain only (no updates at all: wrong factor) -- the floor of the dependency chain
namespace v2 {
template <int M, int J> __device__ __forceinline__ void chol_columns(double (&a)[M], double (&rinv)[M], int& ok, int lane, double dloc)
{
    if constexpr (J < M) {
        const double d = rowbcast_f64<J>(dloc);
        if (!(d > 0.0)) ok = 0;
        const double num = (lane == J) ? d : a[J];
        const double y = fast_rsqrt(d);
        rinv[J] = y;
        const double lij = num * y;
        a[J] = lij;
        double dnext = 0.0;
        if constexpr (J + 1 < M) dnext = fma(-lij, lij, a[J + 1]);
        chol_columns<M, J + 1>(a, rinv, ok, lane, dnext);
    }
}
}
// v3: updates only (no rsq chain: r = 1) -- the issue cost of the 66 updates
namespace v3 {
template <int M, int J, int K> __device__ __forceinline__ void chol_update(double (&a)[M], double lij)
{
    if constexpr (K < M) { a[K] = fma(-lij, rowbcast_f64<K>(lij), a[K]); chol_update<M, J, K + 1>(a, lij); }
}
template <int M, int J> __device__ __forceinline__ void chol_columns(double (&a)[M], int lane)
{
    if constexpr (J < M) { const double lij = a[J]; v0::chol_update<M, J, J + 1>(a, lij); chol_columns<M, J + 1>(a, lane); }
}
}
template <int M, int V>
__global__ void chol(const double* A, double* Lout, long long* cyc, int reps)
{
    __shared__ double sA[M * M], sL[M * M], sr[M];
    const int lane = threadIdx.x;
    for (int i = lane; i < M * M; i += 64) { sA[i] = A[i]; sL[i] = 0.0; }
    __syncthreads();
    long long best = 1ll << 60;
    for (int rep = 0; rep < reps; ++rep) {
        SB(); const long long t0 = clock64(); SB();
        double a[M];
#pragma unroll
        for (int k = 0; k < M; ++k) a[k] = (lane < M) ? sA[lane * M + k] : 0.0;
        double rinv[M]; int ok = 1;
        if constexpr (V == 0) v0::chol_columns<M, 0>(a, rinv, ok, lane);
        if constexpr (V == 1) v1::chol_columns<M, 0>(a, rinv, ok, lane, a[0], 0.0);
        if constexpr (V == 2) v2::chol_columns<M, 0>(a, rinv, ok, lane, a[0]);
        if constexpr (V == 3) { v3::chol_columns<M, 0>(a, lane); for (int k = 0; k < M; ++k) rinv[k] = 1.0; }
        if (lane < M) {
#pragma unroll
            for (int k = 0; k < M; ++k) if (k <= lane) sL[lane * M + k] = a[k];
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < M; ++k) sr[k] = rinv[k];
            sr[0] += ok;
        }
        __syncthreads();
        SB(); const long long t1 = clock64(); SB();
        if (t1 - t0 < best) best = t1 - t0;
    }
    if (lane == 0) cyc[0] = best;
    for (int i = lane; i < M * M; i += 64) Lout[i] = sL[i];
}
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("hip error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)
int main()
{
    double *dA, *dL, *dout; long long* dc;
    CK(hipMalloc(&dA, 144 * 8)); CK(hipMalloc(&dL, 144 * 8)); CK(hipMalloc(&dout, 64 * 8)); CK(hipMalloc(&dc, 16 * 8));
    double A[144], B[144];
    srand(1);
    for (int i = 0; i < 144; ++i) B[i] = rand() / (double)RAND_MAX - 0.5;
    for (int i = 0; i < 12; ++i) for (int j = 0; j < 12; ++j) { double s = (i == j) ? 1.0 : 0.0; for (int k = 0; k < 12; ++k) s += B[i * 12 + k] * B[j * 12 + k]; A[i * 12 + j] = s * 1e-3; }
    CK(hipMemcpy(dA, A, sizeof A, hipMemcpyHostToDevice));
    long long c[16];
    double L0[144], L1[144];
#define RUN(M, V, dst) do { chol<M, V><<<1, 64>>>(dA, dL, dc, 6); CK(hipDeviceSynchronize()); CK(hipMemcpy(c, dc, 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(dst, dL, 144 * 8, hipMemcpyDeviceToHost)); printf("chol M=%d variant %d: %lld cycles (best of 6, incl. LDS load/store + barrier)\n", M, V, c[0]); } while (0)
    RUN(12, 0, L0); RUN(12, 1, L1);
    int same = 1; for (int i = 0; i < 144; ++i) if (L0[i] != L1[i]) same = 0;
    printf("12x12 factor v0 == v1 bit for bit: %d\n", same);
    double tmp[144];
    RUN(12, 2, tmp); RUN(12, 3, tmp);
    return 0;
}
