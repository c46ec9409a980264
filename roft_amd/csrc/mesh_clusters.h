// mesh_clusters.h -- the triangles of a mesh cut into clusters of at most 64 triangles over at most 64 distinct vertices: what one
// wave of the outlier test (outlier_fused_kernel<false>, draw_clusters of k_render.hip) projects and draws at a time.  Host side except for
// cluster_faces_away, which the kernel shares with the CPU test (tests/cpp/cluster_check.cpp compiles this header without HIP).
//
// A cluster is grown inside one of the 24 normal-direction buckets of a closed mesh's walk order (mesh_class.h) -- it never crosses
// into another -- from the bucket's lowest free triangle over triangles that share vertices with it, so that its triangles reuse
// its vertex slots; every triangle is in exactly one cluster.  The render does not depend on the order in which triangles are
// drawn (nearest depth per pixel).  On the device a cluster is
//   * 64 vertex slots, structure of arrays: x[64] | y[64] | z[64], bit copies of the mesh's floats (spare slots repeat slot 0);
//   * 64 triangle words: three 6-bit slot numbers (corner k in bits 6k .. 6k + 5, the triangle's own corner order) and the flip bit of
//     mesh_class.h in bit 18 (spare words are 0: slot 0 three times, a triangle of zero area, which the rasteriser drops);
//   * a header of sixteen 32-bit words (kClusterWords below): the counts and, for a closed mesh, a normal cone with the bounding sphere.
// Slots and words sit at 64 x the cluster's index, so a wave fetches the next cluster without having read its header.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#if defined(__HIPCC__)
#define ROFT_CLUSTER_HD __host__ __device__
#else
#define ROFT_CLUSTER_HD
#endif

namespace roft {

constexpr int kClusterSize = 64;    // triangles and vertex slots of a cluster: one per lane of a wave
constexpr int kClusterWords = 16;   // 32-bit words of a header
// header words (floats as their bit patterns)
enum ClusterWord {
    kCwVerts = 0, kCwTris = 1, kCwCone = 2 /* 1: words 4 .. 14 hold a cone */, kCwBucket = 3,
    kCwAxis = 4 /* 3 */, kCwCos = 7, kCwSin = 8, kCwCenter = 9 /* 3 */, kCwRadius = 12, kCwAreaMin = 13, kCwEdgeMax = 14,
};

ROFT_CLUSTER_HD inline uint32_t pack_cluster_triangle(int s0, int s1, int s2, int flip)
{
    return (uint32_t)s0 | ((uint32_t)s1 << 6) | ((uint32_t)s2 << 12) | ((uint32_t)(flip ? 1 : 0) << 18);
}

// Does every triangle of a cluster of a CLOSED mesh face away from the camera -- so surely that raster_projected's own rule, the
// sign of the screen area it computes in float from the float projections of project_vertex, culls each of them?  May say no for
// a cluster that does; never says yes for one that holds a triangle the rule would draw.  The caller asks only while the
// back-face rule is on (every vertex in front of the near plane), the focal lengths are positive and pose_is_rotation(R).
//   axis, cos_t, sin_t: every outward unit normal n of the cluster has n . axis >= cos_t > 0 (sin_t >= sin of that angle)
//   center, radius:     every vertex of the cluster lies in that sphere (object space)
//   a_min, e_max:       smallest |e1 x e2| (twice the area) and longest edge among its triangles
//   R, t:               the pose as the rasteriser uses it (eye = R v + t); f_lo / f_hi: the smaller / larger of fx, fy;
//   c_abs:              |cx| + |cy|
// Derivation.  v = R center + t, L = |v|, D = L + radius bounds the distance of every vertex, Z = v.z - radius its depth from
// below.  With phi the angle between v and the axis and theta the cone's half angle, a normal n and a point p = v + radius u of
// the cluster give  n . p >= L cos(phi + theta) - radius =: m  (phi + theta < 90 degrees when that is positive): the camera lies
// at least m BEHIND the plane of every triangle.  Exactly, a triangle's screen area is  fx fy (e1 x e2) . a0 / (z0 z1 z2)  -- positive
// for a counter-clockwise triangle seen from behind --, so  |area| >= f_lo^2 a_min m / D^3.  The float area errs by at most
//   4 d (|e1| + |e2|) + 8 d^2 + 8 u |e1| |e2|   (d: error of a screen coordinate, u = 2^-24, e: screen edges),
// a screen edge is at most  f_hi e_max sqrt(2) D / Z^2  long, and a coordinate  s = (f X) (1 / z) + c  computed from sums of
// magnitude up to Dm (below) errs by at most  7 u f_hi (Dm / Z) (1 + D / Z) + u c_abs < d  as taken here (c enters only through the
// rounding of the last sum).  The sign of the float
// area is the exact one while |area| exceeds that error; the test asks for twice as much, and takes the rounding of its own
// arithmetic (a few u Dm on v, L, Z, m) off m.
// ASSUMPTION: R is a rotation.  All of the above -- normals carried as R n, the cone's angle and the sphere's radius kept, the area
// formula's a_min -- holds for a rigid motion only, and make_pose builds R from the caller's quaternion AS GIVEN: a quaternion that
// is not of unit length gives a mix of the identity and a rotation, under which the per-triangle sign of area still means what it meant (any linear
// map) but the cone does not.  The caller asks only where pose_is_rotation(R) holds; its tolerance (entries of R R^T - I within
// 2e-6: singular values within 3e-6 of 1) moves lengths by at most 3e-6 D and a normal by at most 6e-6 radians, together less than
// 1e-5 D on m, which the 2.4e-5 Dm taken off m covers next to the rounding.
ROFT_CLUSTER_HD inline bool cluster_faces_away(float ax0, float ax1, float ax2, float cos_t, float sin_t, float c0, float c1, float c2,
                                               float radius, float a_min, float e_max, const float* R, const float* t, float f_lo,
                                               float f_hi, float c_abs)
{
    const float vx = ((R[0] * c0 + R[1] * c1) + R[2] * c2) + t[0];
    const float vy = ((R[3] * c0 + R[4] * c1) + R[5] * c2) + t[1];
    const float vz = ((R[6] * c0 + R[7] * c1) + R[8] * c2) + t[2];
    const float ex = (R[0] * ax0 + R[1] * ax1) + R[2] * ax2;
    const float ey = (R[3] * ax0 + R[4] * ax1) + R[5] * ax2;
    const float ez = (R[6] * ax0 + R[7] * ax1) + R[8] * ax2;
    const float L = sqrtf((vx * vx + vy * vy) + vz * vz);
    const float D = L + radius, Z = vz - radius;
    // the largest magnitude a row sum of a vertex's transform can reach (|R_ij| <= 1): what its rounding errors scale with
    const float Dm = fmaxf(D, (fabsf(c0) + fabsf(c1) + fabsf(c2)) + 1.75f * radius + fmaxf(fabsf(t[0]), fmaxf(fabsf(t[1]), fabsf(t[2]))));
    if (!(Z > 0.0f) || !(L > 0.0f)) return false;
    float cphi = ((vx * ex + vy * ey) + vz * ez) / L;
    cphi = fminf(fmaxf(cphi, -1.0f), 1.0f);
    const float sphi = sqrtf(fmaxf(0.0f, 1.0f - cphi * cphi));
    const float m = L * (cphi * cos_t - sphi * sin_t) - radius - 2.4e-5f * Dm;
    if (!(m > 0.0f)) return false;
    const float q = D / Z;
    const float d = 1e-6f * (f_hi * (Dm / Z) * (1.0f + q)) + 2e-7f * c_abs;
    const float edge = f_hi * e_max * 1.4143f * q / Z;
    const float lhs = f_lo * f_lo * a_min * m / (D * D * D);
    const float rhs = 2.0f * (8.0f * d * edge + 8.0f * d * d + 8.0f * 6e-8f * edge * edge);
    return lhs >= rhs;   // (a NaN anywhere: false)
}

// Is R (row-major 3 x 3) a rotation, as closely as cluster_faces_away needs: every entry of R R^T - I within 2e-6 and det R > 0.
// A pose from a unit quaternion in double passes (make_pose rounds nine entries to float: R R^T - I within 4e-7); one from a
// quaternion 1e-6 or more off unit length does not, and its render goes without cones.  NaN: false.
ROFT_CLUSTER_HD inline bool pose_is_rotation(const float* R)
{
    bool ok = true;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            const float g = (R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1]) + R[3 * i + 2] * R[3 * j + 2];
            ok = ok && fabsf(g - (i == j ? 1.0f : 0.0f)) <= 2e-6f;
        }
    const float det = (R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6])) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    return ok && det > 0.0f;
}

struct MeshClusters {
    int n_clusters = 0;
    std::vector<uint32_t> headers;   // kClusterWords per cluster
    std::vector<float> slots;        // 3 x 64 per cluster: x[64] | y[64] | z[64]
    std::vector<uint32_t> words;     // 64 per cluster
    float box[8][3];                 // corners of the mesh's axis-aligned box (corner k: bit 0 -> x, 1 -> y, 2 -> z takes the maximum);
                                     // all NaN when a coordinate of the mesh is not finite
    // host side only (the tests): the triangle of the walk order behind every word and the mesh vertex behind every slot (-1: spare)
    std::vector<int32_t> tri_index;
    std::vector<int32_t> slot_vertex;
};

inline uint32_t cluster_float_bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// tris: the mesh's triangles in the order the kernel is to walk them; flip: null (the mesh is not a closed surface: no cones) or
// a closed mesh's flip bits in that order; bucket: null or the triangles' direction buckets in that order (non-decreasing).
inline void build_clusters(const float* verts, int n_verts, const int32_t* tris, int n_tris, const uint8_t* flip, const uint8_t* bucket,
                           MeshClusters& out)
{
    out = MeshClusters();
    const float nan = std::numeric_limits<float>::quiet_NaN();
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    bool finite = n_verts > 0;
    for (int i = 0; i < n_verts; ++i)
        for (int q = 0; q < 3; ++q) {
            const float c = verts[(size_t)3 * i + q];
            if (!std::isfinite(c)) finite = false;
            if (i == 0 || c < lo[q]) lo[q] = c;
            if (i == 0 || c > hi[q]) hi[q] = c;
        }
    for (int k = 0; k < 8; ++k)
        for (int q = 0; q < 3; ++q) out.box[k][q] = finite ? (((k >> q) & 1) ? hi[q] : lo[q]) : nan;
    std::vector<int32_t> stamp((size_t)std::max(n_verts, 0), -1), slot((size_t)std::max(n_verts, 0), 0);
    // vertex -> its triangles, and every triangle's centroid: a cluster grows from a seed over triangles that share vertices with it
    std::vector<int32_t> v_first((size_t)std::max(n_verts, 0) + 1, 0), v_tris((size_t)3 * std::max(n_tris, 0));
    for (size_t i = 0; i < (size_t)3 * std::max(n_tris, 0); ++i) ++v_first[(size_t)tris[i] + 1];
    for (int i = 0; i < n_verts; ++i) v_first[(size_t)i + 1] += v_first[i];
    {
        std::vector<int32_t> fill(v_first.begin(), v_first.end() - 1);
        for (int t = 0; t < n_tris; ++t)
            for (int k = 0; k < 3; ++k) v_tris[(size_t)fill[tris[(size_t)3 * t + k]]++] = t;
    }
    std::vector<double> centroid((size_t)3 * std::max(n_tris, 0));
    for (int t = 0; t < n_tris; ++t)
        for (int q = 0; q < 3; ++q)
            centroid[(size_t)3 * t + q] = ((double)verts[(size_t)3 * tris[(size_t)3 * t] + q] + verts[(size_t)3 * tris[(size_t)3 * t + 1] + q] +
                                           verts[(size_t)3 * tris[(size_t)3 * t + 2] + q]) / 3.0;
    std::vector<uint8_t> done((size_t)std::max(n_tris, 0), 0);
    std::vector<int32_t> in_frontier((size_t)std::max(n_tris, 0), -1), frontier, members;
    out.tri_index.clear();
    int b0 = 0;
    while (b0 < n_tris) {
      // one direction bucket (a mesh without buckets: all of it) at a time: no cluster crosses into the next
      int b1 = n_tris;
      if (bucket) for (b1 = b0 + 1; b1 < n_tris && bucket[b1] == bucket[b0]; ++b1) {}
      int cursor = b0;   // the lowest triangle of the bucket that may still be free
      for (;;) {
        while (cursor < b1 && done[cursor]) ++cursor;
        if (cursor == b1) break;
        const int c = out.n_clusters++, seed = cursor;
        out.headers.resize((size_t)(c + 1) * kClusterWords, 0u);
        out.slots.resize((size_t)(c + 1) * 3 * kClusterSize, 0.0f);
        out.words.resize((size_t)(c + 1) * kClusterSize, 0u);
        out.slot_vertex.resize((size_t)(c + 1) * kClusterSize, -1);
        out.tri_index.resize((size_t)(c + 1) * kClusterSize, -1);
        int nv = 0, nt = 0;
        frontier.clear();
        members.clear();
        auto fresh_corners = [&](int t) {
            const int32_t* tri = tris + (size_t)3 * t;
            int fresh = 0;
            for (int k = 0; k < 3; ++k) {
                bool seen = stamp[tri[k]] == c;
                for (int j = 0; j < k; ++j) seen = seen || tri[j] == tri[k];
                fresh += seen ? 0 : 1;
            }
            return fresh;
        };
        auto take = [&](int t) {
            const int32_t* tri = tris + (size_t)3 * t;
            int s[3];
            for (int k = 0; k < 3; ++k) {
                const int32_t v = tri[k];
                if (stamp[v] != c) {
                    stamp[v] = c;
                    slot[v] = nv;
                    out.slot_vertex[(size_t)c * kClusterSize + nv] = v;
                    for (int q = 0; q < 3; ++q) out.slots[((size_t)c * 3 + q) * kClusterSize + nv] = verts[(size_t)3 * v + q];
                    ++nv;
                    for (int32_t i = v_first[v]; i < v_first[(size_t)v + 1]; ++i) {
                        const int32_t u = v_tris[i];
                        if (u >= b0 && u < b1 && !done[u] && in_frontier[u] != c) { in_frontier[u] = c; frontier.push_back(u); }
                    }
                }
                s[k] = slot[v];
            }
            out.words[(size_t)c * kClusterSize + nt] = pack_cluster_triangle(s[0], s[1], s[2], flip ? flip[t] : 0);
            out.tri_index[(size_t)c * kClusterSize + nt] = t;
            members.push_back(t);
            done[t] = 1;
            ++nt;
        };
        take(seed);   // (an empty cluster always takes a triangle: three slots at most)
        while (nt < kClusterSize) {
            // the neighbour that needs the fewest new slots, among those the one nearest the seed (compact patches: few vertices
            // per triangle, a small sphere); no neighbour left: the lowest free triangle of the bucket, if it fits
            int best = -1, best_fresh = 4;
            double best_d2 = 0.0;
            size_t keep = 0;
            for (size_t i = 0; i < frontier.size(); ++i) {
                const int u = frontier[i];
                if (done[u]) continue;
                frontier[keep++] = u;
                const int fresh = fresh_corners(u);
                if (nv + fresh > kClusterSize) continue;
                double d2 = 0.0;
                for (int q = 0; q < 3; ++q) {
                    const double dq = centroid[(size_t)3 * u + q] - centroid[(size_t)3 * seed + q];
                    d2 += dq * dq;
                }
                if (fresh < best_fresh || (fresh == best_fresh && (d2 < best_d2 || (d2 == best_d2 && u < best)))) { best = u; best_fresh = fresh; best_d2 = d2; }
            }
            frontier.resize(keep);
            if (best < 0 && frontier.empty()) {
                int u = cursor;
                while (u < b1 && done[u]) ++u;
                if (u < b1 && nv + fresh_corners(u) <= kClusterSize) best = u;
            }
            if (best < 0) break;
            take(best);
        }
        for (int sl = nv; sl < kClusterSize; ++sl)
            for (int q = 0; q < 3; ++q) out.slots[((size_t)c * 3 + q) * kClusterSize + sl] = out.slots[((size_t)c * 3 + q) * kClusterSize];
        uint32_t* h = out.headers.data() + (size_t)c * kClusterWords;
        h[kCwVerts] = (uint32_t)nv;
        h[kCwTris] = (uint32_t)nt;
        h[kCwBucket] = bucket ? bucket[seed] : 0u;
        if (!flip) continue;
        // the cone: outward unit normals in double, their mean direction as the axis, the smallest n . axis less a margin that
        // covers the axis' rounding to float; the sphere about the middle of the cluster's box
        double sum[3] = {0, 0, 0}, a_min = std::numeric_limits<double>::infinity(), e_max = 0.0;
        std::vector<double> normals((size_t)3 * nt);
        bool ok = true;
        for (int k = 0; k < nt && ok; ++k) {
            const int32_t* tri = tris + (size_t)3 * members[k];
            const float *a = verts + (size_t)3 * tri[0], *b = verts + (size_t)3 * tri[1], *cc = verts + (size_t)3 * tri[2];
            const double e1[3] = {(double)b[0] - a[0], (double)b[1] - a[1], (double)b[2] - a[2]};
            const double e2[3] = {(double)cc[0] - a[0], (double)cc[1] - a[1], (double)cc[2] - a[2]};
            const double e3[3] = {(double)cc[0] - b[0], (double)cc[1] - b[1], (double)cc[2] - b[2]};
            double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            if (!(len > 0.0) || !std::isfinite(len)) { ok = false; break; }
            const double sgn = flip[members[k]] ? -1.0 : 1.0;
            for (int q = 0; q < 3; ++q) { normals[(size_t)3 * k + q] = sgn * n[q] / len; sum[q] += sgn * n[q] / len; }
            a_min = std::min(a_min, len);
            for (const double* e : {e1, e2, e3}) e_max = std::max(e_max, std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]));
        }
        const double sl = std::sqrt(sum[0] * sum[0] + sum[1] * sum[1] + sum[2] * sum[2]);
        if (!ok || !(sl > 1e-6 * nt)) continue;
        const float axis[3] = {(float)(sum[0] / sl), (float)(sum[1] / sl), (float)(sum[2] / sl)};
        double cos_t = 1.0;
        for (int k = 0; k < nt; ++k)
            cos_t = std::min(cos_t, normals[(size_t)3 * k] * axis[0] + normals[(size_t)3 * k + 1] * axis[1] + normals[(size_t)3 * k + 2] * axis[2]);
        cos_t -= 1e-6;
        if (!(cos_t > 1e-3)) continue;   // (a cluster that wraps an edge of 90 degrees or more: no cone)
        const double sin_t = std::sqrt(std::max(0.0, 1.0 - cos_t * cos_t)) * (1.0 + 1e-6) + 1e-7;
        float clo[3], chi[3], center[3];
        for (int q = 0; q < 3; ++q) {
            clo[q] = chi[q] = out.slots[((size_t)c * 3 + q) * kClusterSize];
            for (int s2 = 1; s2 < nv; ++s2) {
                clo[q] = std::min(clo[q], out.slots[((size_t)c * 3 + q) * kClusterSize + s2]);
                chi[q] = std::max(chi[q], out.slots[((size_t)c * 3 + q) * kClusterSize + s2]);
            }
            center[q] = 0.5f * clo[q] + 0.5f * chi[q];
        }
        double r2 = 0.0;
        for (int s2 = 0; s2 < nv; ++s2) {
            double d2 = 0.0;
            for (int q = 0; q < 3; ++q) {
                const double dq = (double)out.slots[((size_t)c * 3 + q) * kClusterSize + s2] - center[q];
                d2 += dq * dq;
            }
            r2 = std::max(r2, d2);
        }
        const float radius = (float)(std::sqrt(r2) * (1.0 + 1e-6)), f_amin = (float)(a_min * (1.0 - 1e-6)), f_emax = (float)(e_max * (1.0 + 1e-6));
        if (!std::isfinite(radius) || !(f_amin > 0.0f) || !std::isfinite(f_emax) || !std::isfinite(center[0] + center[1] + center[2])) continue;
        h[kCwCone] = 1u;
        for (int q = 0; q < 3; ++q) { h[kCwAxis + q] = cluster_float_bits(axis[q]); h[kCwCenter + q] = cluster_float_bits(center[q]); }
        h[kCwCos] = cluster_float_bits((float)cos_t);
        h[kCwSin] = cluster_float_bits((float)sin_t);
        h[kCwRadius] = cluster_float_bits(radius);
        h[kCwAreaMin] = cluster_float_bits(f_amin);
        h[kCwEdgeMax] = cluster_float_bits(f_emax);
      }
      b0 = b1;
    }
}

}  // namespace roft
