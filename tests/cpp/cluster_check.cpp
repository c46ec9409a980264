// cluster_check.cpp -- the cluster builder of the outlier test (roft_amd/csrc/mesh_clusters.h) on one mesh, without HIP.
// Built and run by tests/test_mesh_clusters_cpu.py:
//   g++ -std=c++17 -O1 -ffp-contract=off -Wall -Werror -I roft_amd/csrc cluster_check.cpp -x c++ mesh_class.hip
//   cluster_check <mesh file> <poses> <seed> [near]
// mesh file: int32 n_verts, int32 n_tris, float32 verts[3 n_verts], int32 tris[3 n_tris].  Prints one line
//   "cluster_check ok closed=<0|1> clusters=<n> slots=<n> cones=<n> asked=<n> rejected=<n> facing_away=<n> not_rotations=<n>"
// or the first violation, and exits non-zero.
// Checked: every triangle of the walk order is in exactly one cluster; at most 64 triangles and 64 distinct vertices; no
// cluster crosses a direction bucket; the slots are bit copies of the vertices and the unpacked words give back the triangles'
// corners and flip bits; spare slots and words are harmless; the mesh box holds every vertex.  Cone soundness by brute force: for
// seeded poses -- random, grazing (the camera close to the plane of a triangle), close to the surface, and with quaternions that are
// not of unit length (far off: pose_is_rotation must keep the cones from being asked; within its tolerance: asked) -- no cluster that
// cluster_faces_away rejects holds a triangle that the render contract's own area test, restated here in float from the float
// projections, would draw.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "mesh_class.h"
#include "mesh_clusters.h"

using namespace roft;

static int fail(const char* what, long long a = 0, long long b = 0)
{
    std::printf("cluster_check FAILED: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

struct Pose {
    float R[9], t[3];
};

// the contract's vertex projection (oracle/ro_render.c), restated
static void project(const float* v, const Pose& P, float fx, float fy, float cx, float cy, float& sx, float& sy, float& z)
{
    const float X = ((P.R[0] * v[0] + P.R[1] * v[1]) + P.R[2] * v[2]) + P.t[0];
    const float Y = ((P.R[3] * v[0] + P.R[4] * v[1]) + P.R[5] * v[2]) + P.t[1];
    z = ((P.R[6] * v[0] + P.R[7] * v[1]) + P.R[8] * v[2]) + P.t[2];
    if (z > 0.001f) {
        const float iz = 1.0f / z;
        sx = (fx * X) * iz + cx;
        sy = (fy * Y) * iz + cy;
    } else {
        sx = sy = 0.0f;
    }
}

static Pose make_pose(const double* x, const double* q)
{
    Pose p;
    const double w = q[0], qx = q[1], qy = q[2], qz = q[3];
    p.R[0] = (float)(1.0 - 2.0 * (qy * qy + qz * qz)); p.R[1] = (float)(2.0 * (qx * qy - w * qz)); p.R[2] = (float)(2.0 * (qx * qz + w * qy));
    p.R[3] = (float)(2.0 * (qx * qy + w * qz)); p.R[4] = (float)(1.0 - 2.0 * (qx * qx + qz * qz)); p.R[5] = (float)(2.0 * (qy * qz - w * qx));
    p.R[6] = (float)(2.0 * (qx * qz - w * qy)); p.R[7] = (float)(2.0 * (qy * qz + w * qx)); p.R[8] = (float)(1.0 - 2.0 * (qx * qx + qy * qy));
    for (int i = 0; i < 3; ++i) p.t[i] = (float)x[i];
    return p;
}

int main(int argc, char** argv)
{
    if (argc < 4) return fail("usage");
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return fail("mesh file");
    int32_t nv = 0, nt = 0;
    if (std::fread(&nv, 4, 1, f) != 1 || std::fread(&nt, 4, 1, f) != 1 || nv <= 0 || nt <= 0) return fail("header");
    std::vector<float> verts((size_t)3 * nv);
    std::vector<int32_t> tris_in((size_t)3 * nt);
    if (std::fread(verts.data(), 4, verts.size(), f) != verts.size() || std::fread(tris_in.data(), 4, tris_in.size(), f) != tris_in.size())
        return fail("arrays");
    std::fclose(f);
    const int n_poses = std::atoi(argv[2]);
    const bool near_only = argc > 4 && std::strcmp(argv[4], "near") == 0;   // poses at the bench's distances and divider, the mesh in view
    std::mt19937_64 rng((unsigned long long)std::atoll(argv[3]));

    PreparedMesh pm;
    prepare_mesh(verts.data(), nv, tris_in.data(), nt, MeshLayout::kWalkOrder, pm);
    const int32_t* tris = pm.tris(tris_in.data());
    const uint8_t* flip = pm.closed ? pm.flip.data() : nullptr;
    MeshClusters mc;
    build_clusters(verts.data(), nv, tris, nt, flip, pm.bucket.empty() ? nullptr : pm.bucket.data(), mc);

    // ---- structure
    const int nc = mc.n_clusters;
    std::vector<int> times_used((size_t)nt, 0);
    if (mc.tri_index.size() != (size_t)nc * kClusterSize || mc.slot_vertex.size() != (size_t)nc * kClusterSize) return fail("index sizes");
    if (mc.headers.size() != (size_t)nc * kClusterWords || mc.slots.size() != (size_t)nc * 3 * kClusterSize ||
        mc.words.size() != (size_t)nc * kClusterSize)
        return fail("array sizes");
    int cones = 0;
    long long slots_used = 0;
    for (int c = 0; c < nc; ++c) {
        const uint32_t* h = mc.headers.data() + (size_t)c * kClusterWords;
        const int cv = (int)h[kCwVerts], ct = (int)h[kCwTris];
        if (ct < 1 || ct > kClusterSize || cv < 1 || cv > kClusterSize) return fail("counts", c, ct);
        if (!pm.closed && h[kCwCone]) return fail("cone on a mesh that is not closed", c);
        cones += h[kCwCone] ? 1 : 0;
        slots_used += cv;
        for (int s = 0; s < kClusterSize; ++s) {
            const int32_t v = mc.slot_vertex[(size_t)c * kClusterSize + s];
            if ((s < cv) != (v >= 0)) return fail("slot count", c, s);
            for (int s2 = 0; s2 < s && v >= 0; ++s2)
                if (mc.slot_vertex[(size_t)c * kClusterSize + s2] == v) return fail("vertex in two slots", c, v);
            const int src = v >= 0 ? s : 0;   // (spare slots repeat slot 0)
            for (int q = 0; q < 3; ++q) {
                const float got = mc.slots[((size_t)c * 3 + q) * kClusterSize + s];
                const float want = v >= 0 ? verts[(size_t)3 * v + q] : mc.slots[((size_t)c * 3 + q) * kClusterSize + src];
                if (std::memcmp(&got, &want, 4) != 0) return fail("slot is no bit copy", c, s);
            }
        }
        for (int k = 0; k < kClusterSize; ++k) {
            const uint32_t w = mc.words[(size_t)c * kClusterSize + k];
            const int t = mc.tri_index[(size_t)c * kClusterSize + k];
            if (k >= ct) { if (w != 0 || t != -1) return fail("spare word", c, k); continue; }
            if (t < 0 || t >= nt) return fail("triangle index", c, k);
            ++times_used[t];
            if (!pm.bucket.empty() && pm.bucket[t] != pm.bucket[mc.tri_index[(size_t)c * kClusterSize]]) return fail("cluster crosses a bucket", c, t);
            if (!pm.bucket.empty() && h[kCwBucket] != pm.bucket[t]) return fail("bucket word", c, t);
            for (int q = 0; q < 3; ++q) {
                const int s = (int)((w >> (6 * q)) & 63u);
                if (s >= cv || mc.slot_vertex[(size_t)c * kClusterSize + s] != tris[(size_t)3 * t + q]) return fail("corner", t, q);
            }
            if (((w >> 18) & 1u) != (flip ? flip[t] : 0u) || (w >> 19) != 0) return fail("flip bit", t);
        }
    }
    for (int t = 0; t < nt; ++t)
        if (times_used[t] != 1) return fail("triangle not in exactly one cluster", t, times_used[t]);
    bool finite = true;
    for (float c : verts) finite = finite && std::isfinite(c);
    for (int i = 0; i < nv && finite; ++i)
        for (int q = 0; q < 3; ++q)
            if (verts[(size_t)3 * i + q] < mc.box[0][q] || verts[(size_t)3 * i + q] > mc.box[7][q]) return fail("vertex outside the box", i, q);
    for (int k = 0; k < 8; ++k)
        for (int q = 0; q < 3; ++q)
            if (finite ? mc.box[k][q] != mc.box[((k >> q) & 1) ? 7 : 0][q] : !std::isnan(mc.box[k][q])) return fail("box corner", k, q);

    // ---- cone soundness
    long long asked = 0, rejected = 0, facing_away = 0, unguarded = 0;
    if (pm.closed) {
        double lo[3], hi[3];
        for (int q = 0; q < 3; ++q) { lo[q] = mc.box[0][q]; hi[q] = mc.box[7][q]; }
        const double size = std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
        std::normal_distribution<double> gauss(0.0, 1.0);
        std::uniform_real_distribution<double> uni(0.0, 1.0);
        std::vector<float> sx((size_t)nv), sy((size_t)nv), sz((size_t)nv);
        for (int p = 0; p < n_poses; ++p) {
            double q[4];
            double qn = 0.0;
            for (double& e : q) { e = gauss(rng); qn += e * e; }
            for (double& e : q) e /= std::sqrt(qn);
            const int kind = near_only ? 0 : p % 4;   // 0, 1: anywhere in front; 2: grazing a triangle's plane; 3: close to the surface
            // the camera's place in OBJECT space -> the translation that puts it there: eye = R (v - cam)
            double cam[3];
            const int t = (int)(uni(rng) * nt) % nt;
            const float *a = &verts[(size_t)3 * tris[3 * t]], *b = &verts[(size_t)3 * tris[3 * t + 1]], *c = &verts[(size_t)3 * tris[3 * t + 2]];
            const double e1[3] = {(double)b[0] - a[0], (double)b[1] - a[1], (double)b[2] - a[2]}, e2[3] = {(double)c[0] - a[0], (double)c[1] - a[1], (double)c[2] - a[2]};
            double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            const double nl = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) * (flip[t] ? -1.0 : 1.0);
            for (double& e : n) e /= nl;
            if (kind < 2) {
                double d[3], dl = 0.0;
                for (double& e : d) { e = gauss(rng); dl += e * e; }
                const double dist = near_only ? size * (1.5 + 1.5 * uni(rng)) : size * (0.8 + 6.0 * uni(rng));
                for (int k = 0; k < 3; ++k) cam[k] = 0.5 * (lo[k] + hi[k]) + d[k] / std::sqrt(dl) * dist;
            } else if (kind == 2) {
                // in the triangle's plane, a few edge lengths to many object sizes away, lifted off it by a tiny signed angle
                const double along = uni(rng), dist = size * (0.6 + 4.0 * uni(rng)), lift = dist * (uni(rng) - 0.5) * (p % 8 < 4 ? 1e-2 : 1e-5);
                const double el = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]), fl = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
                for (int k = 0; k < 3; ++k) cam[k] = a[k] + dist * (along * e1[k] / el + (1.0 - along) * e2[k] / fl) + lift * n[k];
            } else {
                const double h2 = size * (0.02 + 0.3 * uni(rng));   // above the triangle, outside
                for (int k = 0; k < 3; ++k) cam[k] = (a[k] + b[k] + c[k]) / 3.0 + h2 * n[k];
            }
            Pose P = make_pose(cam, q);   // (rotation only: t is set below)
            if (kind >= 2 || near_only) {
                // look at the triangle (near: at a point about the middle of the mesh): any rotation whose third row points from the
                // camera to it
                double target[3] = {a[0], a[1], a[2]};
                if (near_only)
                    for (int k = 0; k < 3; ++k) target[k] = 0.5 * (lo[k] + hi[k]) + 0.3 * size * (uni(rng) - 0.5);
                double z[3] = {target[0] - cam[0], target[1] - cam[1], target[2] - cam[2]}, zl = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
                for (double& e : z) e /= zl;
                double u[3] = {gauss(rng), gauss(rng), gauss(rng)};
                const double uz = u[0] * z[0] + u[1] * z[1] + u[2] * z[2];
                double ul = 0.0;
                for (int k = 0; k < 3; ++k) { u[k] -= uz * z[k]; ul += u[k] * u[k]; }
                for (double& e : u) e /= std::sqrt(ul);
                const double w[3] = {z[1] * u[2] - z[2] * u[1], z[2] * u[0] - z[0] * u[2], z[0] * u[1] - z[1] * u[0]};
                for (int k = 0; k < 3; ++k) { P.R[k] = (float)u[k]; P.R[3 + k] = (float)w[k]; P.R[6 + k] = (float)z[k]; }
            }
            // every fifth pose: the rotation a quaternion of length k != 1 gives, (1 - k^2) I + k^2 R (make_pose takes a quaternion as it
            // is given).  Two are far from a rotation -- pose_is_rotation must say so and the kernel does not ask the cones --, two
            // within its tolerance, where the cones are asked and must stay sound.
            if (!near_only && p % 5 == 4) {
                const double k2s[4] = {1.0 / (0.98 * 0.98), 1.002, 1.0 + 8e-7, 1.0 - 8e-7};
                const double k2 = k2s[(p / 5) % 4];
                for (int i = 0; i < 9; ++i) P.R[i] = (float)(k2 * P.R[i] + ((i % 4 == 0) ? 1.0 - k2 : 0.0));
                if ((p / 5) % 4 < 2 && pose_is_rotation(P.R)) return fail("pose_is_rotation accepts the pose of a quaternion 0.1 % off unit length", p);
            }
            for (int r = 0; r < 3; ++r) P.t[r] = (float)-(P.R[3 * r] * cam[0] + P.R[3 * r + 1] * cam[1] + P.R[3 * r + 2] * cam[2]);
            const int div = near_only ? 2 : ((p % 3 == 0) ? 1 : (p % 3 == 1 ? 2 : 4));
            const float fx = (float)(614.0 / div), fy = (float)(611.0 / div), cx = (float)(321.5 / div), cy = (float)(238.25 / div);
            bool behind = false;
            for (int i = 0; i < nv; ++i) {
                project(&verts[(size_t)3 * i], P, fx, fy, cx, cy, sx[i], sy[i], sz[i]);
                behind = behind || !(sz[i] > 0.001f);
            }
            if (behind) continue;   // (the back-face rule is off: the kernel does not ask)
            const bool rotation = pose_is_rotation(P.R);   // (else the kernel does not ask either)
            unguarded += rotation ? 0 : 1;
            for (int cl = 0; cl < nc; ++cl) {
                const uint32_t* h = mc.headers.data() + (size_t)cl * kClusterWords;
                // what the contract's area test does with the cluster's triangles
                bool drawn = false;
                for (int k = 0; k < (int)h[kCwTris]; ++k) {
                    const int tt = mc.tri_index[(size_t)cl * kClusterSize + k];
                    const int v0 = tris[3 * tt], v1 = tris[3 * tt + 1], v2 = tris[3 * tt + 2];
                    const float area = (sx[v1] - sx[v0]) * (sy[v2] - sy[v0]) - (sx[v2] - sx[v0]) * (sy[v1] - sy[v0]);
                    if (area == 0.0f || !(area == area)) continue;
                    const int cull = 1 + flip[tt];
                    if ((area < 0.0f) == (cull == 2)) continue;
                    drawn = true;
                }
                facing_away += drawn ? 0 : 1;
                if (!h[kCwCone] || !rotation) continue;
                ++asked;
                float hf[kClusterWords];
                std::memcpy(hf, h, sizeof(hf));
                const bool away = cluster_faces_away(hf[kCwAxis], hf[kCwAxis + 1], hf[kCwAxis + 2], hf[kCwCos], hf[kCwSin], hf[kCwCenter], hf[kCwCenter + 1],
                                                     hf[kCwCenter + 2], hf[kCwRadius], hf[kCwAreaMin], hf[kCwEdgeMax], P.R, P.t, std::fmin(fx, fy),
                                                     std::fmax(fx, fy), std::fabs(cx) + std::fabs(cy));
                if (away && drawn) return fail("the cone rejects a cluster with a triangle the area test draws", p, cl);
                rejected += away ? 1 : 0;
            }
        }
    }
    std::printf("cluster_check ok closed=%d clusters=%d slots=%lld cones=%d asked=%lld rejected=%lld facing_away=%lld not_rotations=%lld\n", pm.closed ? 1 : 0, nc, slots_used, cones,
                asked, rejected, facing_away, unguarded);
    return 0;
}
