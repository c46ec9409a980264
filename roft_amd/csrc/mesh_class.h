// mesh_class.h -- host side, no device code: does a caller's mesh exist and do its triangles name vertices it has, is it a closed
// orientable surface, which triangles are wound inwards, and the arrays in which it goes up to the device (mesh_class.hip).
#pragma once

#include <cstdint>
#include <vector>

namespace roft {

// "The object has a mesh": both counts positive.  Anything with n_verts / n_tris will do (roft_mesh, ObjParams).
inline bool has_mesh(int n_verts, int n_tris) { return n_verts > 0 && n_tris > 0; }
template <class M>
inline bool has_mesh(const M& m) { return has_mesh(m.n_verts, m.n_tris); }

// What is wrong with the arrays of a mesh that has_mesh: nothing, a null array, or the first triangle corner that is no vertex of
// the mesh (the rasteriser indexes the vertex array with these).  The caller words the refusal ("mesh 3: ...").
struct MeshFault {
    enum Kind { kFine, kNullArray, kBadIndex } kind = kFine;
    long long triangle = 0;   // kBadIndex: the triangle ...
    int32_t vertex = 0;       // ... and the vertex it refers to
    explicit operator bool() const { return kind != kFine; }
};
MeshFault check_mesh_arrays(const float* verts, int n_verts, const int32_t* tris, int n_tris);

// The render contract's classification (oracle/ro_meshclass.c states the rules; this is the engine's own implementation of
// them): true and flip[t] = 1 for every triangle wound clockwise seen from outside when the mesh is a closed orientable
// surface; false (flip zeroed) for anything else -- such a mesh is drawn whole, exactly as the reference draws every mesh
// (depth test LESS, no culling: src/roft-lib/src/SICAD.cpp:271-272).
bool classify_mesh(const float* verts, int n_verts, const int32_t* tris, int n_tris, std::vector<uint8_t>& flip);

// The device copy of a CLOSED mesh's triangles: the same triangles (vertex order inside a triangle untouched -- the per-pixel
// arithmetic depends on it), reordered so that triangles whose outward normals point alike are neighbours (24 direction
// buckets: cube face x 2 x 2).  The render's result does not depend on the order (nearest depth per pixel); the order decides
// which triangles share a wave, and a wave whose 64 triangles all face away is skipped whole.  order[k] = index of the
// triangle walked k-th; bucket_of (optional): the direction bucket, 0 .. 23, of every triangle in the CALLER's order.
void facing_coherent_order(const float* verts, const int32_t* tris, int n_tris, const std::vector<uint8_t>& flip, std::vector<int32_t>& order,
                           std::vector<uint8_t>* bucket_of = nullptr);

// The layouts in which a mesh goes up.  A mesh that is not closed goes up as the caller's triangles, without flip bits, in all of them.
enum class MeshLayout {
    kWalkOrder,     // closed: the triangles in the facing-coherent order, flip bits in that order (the operators that walk `tris`)
    kWalkClusters,  // kWalkOrder, and the device copy also holds those triangles as clusters (mesh_clusters.h): every mesh the contract
                    // render of the outlier test draws -- that kernel walks the clusters and nothing else
    kCallersOrder,  // closed: the caller's triangles, flip bits in the caller's order (the scene renderer: a key's triangle index is the caller's)
    kAsItIs,        // never classified: the caller's triangles, no flip bits (the GL render mode draws every triangle, ties by the caller's order)
};
struct PreparedMesh {
    bool closed = false;
    std::vector<int32_t> reordered;   // 3 x n_tris: closed meshes in walk order only
    std::vector<uint8_t> flip;        // n_tris: closed meshes only, in the order of tris()
    std::vector<uint8_t> bucket;      // n_tris: closed meshes in walk order only, the direction bucket of every triangle of tris() (mesh_clusters.h)
    const int32_t* tris(const int32_t* callers) const { return reordered.empty() ? callers : reordered.data(); }
};
void prepare_mesh(const float* verts, int n_verts, const int32_t* tris, int n_tris, MeshLayout layout, PreparedMesh& out);

}  // namespace roft
