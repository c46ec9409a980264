// raster_shape.h -- the LDS arithmetic of a launcher whose workgroups draw a mesh into an LDS window (raster.h): host only, no HIP
// include (tests/cpp/raster_shape_check.cpp compares every launcher's rule below with tests/golden/raster_shapes.json).
// raster_shape() is the rule of the launchers whose strips are whole rows (quality, VSD); the scene renderer's stands next to it.
// Dynamic LDS of such a workgroup: [the projected vertices, when they are cached] | [its window, or its windows side by side].
#pragma once

#include <algorithm>
#include <cstddef>

namespace roft {

constexpr size_t kRasterLdsBudget = 160 * 1024 - 4096;   // what such a kernel may ask for (the rest: its static LDS)
constexpr size_t vertex_cache_bytes(int verts) { return ((size_t)verts * 12 + 15) & ~(size_t)15; }   // = the window's offset

struct RasterShape {
    bool ok;          // false: not even one row of the target fits (nothing may be launched; vcache_cap aside, the rest is 0)
    int vcache_cap;   // vertices the cache holds (0: every triangle projects its own corners)
    int win_alloc;    // pixels each window has room for ...
    int win_cap;      // ... and how many of them a strip may use (window_pixels: operator level, forces strips)
    size_t lds;       // bytes to ask for
};

// n_verts: the largest mesh.  row: pixels of the widest row a strip must hold.  pixel_bytes: bytes
// of a window element x windows.  cache_min: the vertices are cached only where they leave room for windows of this many pixels.
// cap: pixels of a window when there is room for more.  window_pixels > 0 lowers win_cap, not below win_floor, and leaves the
// allocation as it is: a strip of one row is at most `row` <= the allocation wide.
inline RasterShape raster_shape(int n_verts, size_t row, size_t pixel_bytes, size_t cache_min, size_t cap, int window_pixels, int win_floor)
{
    RasterShape sh = {false, 0, 0, 0, 0};
    const size_t vbytes = vertex_cache_bytes(n_verts);
    const size_t cache_bytes = vbytes + pixel_bytes * cache_min <= kRasterLdsBudget ? vbytes : 0;
    sh.vcache_cap = cache_bytes ? n_verts : 0;
    const size_t room = (kRasterLdsBudget - cache_bytes) / pixel_bytes;   // pixels per window
    if (row > room) return sh;
    sh.ok = true;
    sh.win_alloc = sh.win_cap = (int)std::min(room, cap);
    sh.lds = cache_bytes + pixel_bytes * (size_t)sh.win_alloc;
    if (window_pixels > 0) sh.win_cap = std::max(win_floor, std::min(sh.win_cap, window_pixels));
    return sh;
}

// quality_body.h (track quality, pose hypotheses): the projected vertices of the largest mesh where they leave room for a window of
// 8 k depths, and a window of 16 k pixels (an object's window is about 70 x 90 of 320 x 240 at the metric shape; a larger one is
// drawn in strips) -- not the whole LDS, so that workgroups of the chains the launch runs next to still find a place on the CU.
// A capped window still holds one row of the target.
inline RasterShape quality_window_shape(int max_verts, int tile_w, int window_pixels)
{
    return raster_shape(max_verts, (size_t)tile_w, 4, std::max<size_t>(8192, tile_w), std::max<size_t>(16384, tile_w), window_pixels, tile_w);
}

// k_vsd.hip: the projected vertices where they leave room for two windows of 4 k pixels, and two windows of at most 16 k pixels (an
// object of a tracked sequence covers a few tens of thousands of pixels at 640 x 480: a handful of strips).  A capped strip holds
// at least one row all the same (the kernel's strip_rows).
inline RasterShape vsd_shape(int n_verts, int width, int window_pixels)
{
    return raster_shape(n_verts, (size_t)width, 2 * 4, std::max<size_t>(4096, width), std::max<size_t>(16384, width), window_pixels, 0);
}

// k_scene.hip, a rule of its own: its kernel cuts rows into column runs, so no target is refused and no row must fit, and a capped
// window asks only for the LDS it uses.  The projected vertices when they leave room for a window of 8 k keys, and the window.
// 8 k keys = 64 KB: two workgroups share a CU.  (A larger window means fewer strips, each of which walks all triangles, but one
// workgroup per CU; the object of a tracked sequence covers a few tens of thousands of pixels, a handful of strips.)
inline RasterShape scene_window_shape(int max_verts, size_t target_pixels, int window_pixels)
{
    size_t win = std::min<size_t>(target_pixels, 8192);
    const size_t vbytes = vertex_cache_bytes(max_verts);
    const size_t cache_bytes = vbytes + 8 * win <= kRasterLdsBudget ? vbytes : 0;
    if (window_pixels > 0) win = std::min<size_t>(win, (size_t)window_pixels);
    return RasterShape{true, cache_bytes ? max_verts : 0, (int)win, (int)win, cache_bytes + 8 * win};
}

}  // namespace roft
