// symmetry.h -- discrete symmetry groups of an object (include/roft_engine.h, section 3h): the check of a group, the selection of
// the equivalent pose nearest to a belief, and the transform of a group element.  Plain arithmetic, no HIP call: the pose UKF
// (k_ukf.hip), the scoring kernel (k_metrics.hip) and the host operator roft_pose_nearest_equivalent (engine_ops.hip) include
// this one text.  Every product and every sum is one rounded double operation (the library is built with -ffp-contract=off, as
// is every program that includes this header for a comparison of bits).
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define ROFT_SYM_HD __host__ __device__
#else
#define ROFT_SYM_HD
#endif

namespace roft {
namespace sym {

constexpr int kMaxFilter = 16;    // ROFT_MAX_SYMMETRIES
constexpr int kMaxScore = 256;    // ROFT_MAX_SCORE_SYMMETRIES
constexpr int kElement = 7;       // doubles per element: x y z, w x y z

// Hamilton product a (x) b, quaternions w x y z; the four terms of each component summed left to right
ROFT_SYM_HD inline void quat_mul(double a0, double a1, double a2, double a3, double b0, double b1, double b2, double b3, double& o0,
                                 double& o1, double& o2, double& o3)
{
    o0 = a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3;
    o1 = a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2;
    o2 = a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1;
    o3 = a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0;
}

ROFT_SYM_HD inline double quat_dot(double a0, double a1, double a2, double a3, double b0, double b1, double b2, double b3)
{
    return a0 * b0 + a1 * b1 + a2 * b2 + a3 * b3;
}

// c_g = | qh . (m (x) g) | for the element whose quaternion is g[0..3]; a c_g that is not a number counts as -1, so that an
// input without a meaning never takes the choice away from the identity
ROFT_SYM_HD inline double closeness(const double* qh, const double* m, const double* g)
{
    double p0, p1, p2, p3;
    quat_mul(m[0], m[1], m[2], m[3], g[0], g[1], g[2], g[3], p0, p1, p2, p3);
    const double c = fabs(quat_dot(qh[0], qh[1], qh[2], qh[3], p0, p1, p2, p3));
    return c == c ? c : -1.0;
}

// (value, index) order of the arg-max: the larger value, and the lower index among equal values
ROFT_SYM_HD inline bool better(double c, int g, double than_c, int than_g) { return c > than_c || (c == than_c && g < than_g); }

// metrics.quat_to_rot, operation by operation (the order of load_pose in k_metrics.hip)
ROFT_SYM_HD inline void quat_to_rot(double w, double x, double y, double z, double R[9])
{
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// The measurement (x, m) moved by the NON-IDENTITY element el (7 doubles): m' = m (x) g, negated in all four components when
// qh . m' < 0; x' = x + R(m) t, every row of R(m) t summed left to right.  xq: x' y' z', w' x' y' z' (7 doubles).
ROFT_SYM_HD inline void apply(const double* qh, const double* x, const double* m, const double* el, double* xq)
{
    double p0, p1, p2, p3;
    quat_mul(m[0], m[1], m[2], m[3], el[3], el[4], el[5], el[6], p0, p1, p2, p3);
    if (quat_dot(qh[0], qh[1], qh[2], qh[3], p0, p1, p2, p3) < 0.0) { p0 = -p0; p1 = -p1; p2 = -p2; p3 = -p3; }
    double R[9];
    quat_to_rot(m[0], m[1], m[2], m[3], R);
    const double t0 = el[0], t1 = el[1], t2 = el[2];
    xq[0] = x[0] + (R[0] * t0 + R[1] * t1 + R[2] * t2);
    xq[1] = x[1] + (R[3] * t0 + R[4] * t1 + R[5] * t2);
    xq[2] = x[2] + (R[6] * t0 + R[7] * t1 + R[8] * t2);
    xq[3] = p0; xq[4] = p1; xq[5] = p2; xq[6] = p3;
}

// the element the rule chooses, by the serial form of the arg-max (the kernel's shuffle tree uses better() and finds the same one)
inline int select(const double* sym, int n, const double* qh, const double* m)
{
    int best = 0;
    double best_c = closeness(qh, m, sym + 3);
    for (int g = 1; g < n; ++g) {
        const double c = closeness(qh, m, sym + kElement * g + 3);
        if (better(c, g, best_c, best)) { best = g; best_c = c; }
    }
    return best;
}

// The host check of a group of n elements against a cap; null: the group is accepted, else the reason.
inline const char* check(const double* sym, int n, int cap)
{
    if (!sym) return "symmetry group: null array";
    if (n < 1 || n > cap) return "symmetry group: the number of elements is outside 1 .. the cap";
    for (int i = 0; i < kElement * n; ++i)
        if (!std::isfinite(sym[i])) return "symmetry group: a component is not finite";
    static const double identity[kElement] = {0, 0, 0, 1, 0, 0, 0};
    for (int i = 0; i < kElement; ++i)
        if (sym[i] != identity[i]) return "symmetry group: element 0 must be exactly the identity 0 0 0 1 0 0 0";
    for (int g = 0; g < n; ++g) {
        const double* q = sym + kElement * g + 3;
        const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        if (!(fabs(n2 - 1.0) <= 1e-6)) return "symmetry group: an element's quaternion is not of unit length (| |q|^2 - 1 | <= 1e-6)";
    }
    return nullptr;
}

}  // namespace sym
}  // namespace roft
