// srbh_head_walk.h -- the head kernels' XCD-aware tile walk and tile decode, written once (included by srbh_head.hip and srbh_head_bwd.hip).
//
// Workgroups are dealt round-robin to the 8 XCDs (blockIdx % 8), each with its own L2.  Consecutive tiles (x-neighbours, then the next tile
// row) share halo rows -- 55 % more input rows than a tile owns at 4-row tiles -- so XCD x owns the contiguous tiles [x * tiles_per_xcd,
// (x + 1) * tiles_per_xcd) and the halo re-reads hit that XCD's L2 instead of going out to the fabric.  Its gridDim / 8 workgroups sweep that
// run side by side: workgroup j of the XCD takes tiles j, j + gridDim / 8, ... up to the run's end (the last run is clipped by ntiles; a
// workgroup whose range is empty does nothing).  With gridDim = 8 * tiles_per_xcd this is one tile per workgroup (hconv_f32_kernel); the
// persistent kernels launch min(tiles_per_xcd, cap / 8) workgroups per XCD (srbh_internal.h: head_set_tiles / head_walk_grid).
//
// P is any parameter struct with tiles_x / tiles_per_img / ntiles / tiles_per_xcd.  All forced inline.  How P is passed is part of the
// record (profiles/head_launch_path_isa.txt): the persistent kernels compile to their hand-written instructions with P BY REFERENCE,
// hconv_f32_kernel only with the by-value decode (head_tile_v); the weight-gradient family keeps its own by-value wg_walk / wg_tile
// (srbh_hwgrad_b16_kernel.h), which by reference changed four of its forms.
#pragma once

// the calling workgroup's first tile, the end of its XCD's run and the distance between its tiles
template <class P>
__device__ __forceinline__ void head_walk(const P& p, int& t_first, int& t_end, int& t_step) {
    t_end = min((int)(blockIdx.x & 7) * p.tiles_per_xcd + p.tiles_per_xcd, p.ntiles);
    t_first = (blockIdx.x & 7) * p.tiles_per_xcd + (blockIdx.x >> 3);
    t_step = gridDim.x >> 3;
}

// tile t -> image, tile row, tile column
template <class P>
__device__ __forceinline__ void head_tile(const P& p, const int t, int& img, int& ty, int& tx) {
    img = t / p.tiles_per_img;
    const int trem = t - img * p.tiles_per_img;
    ty = trem / p.tiles_x;
    tx = trem - ty * p.tiles_x;
}
template <class P>
__device__ __forceinline__ void head_tile_v(const P p, const int t, int& img, int& ty, int& tx) { head_tile(p, t, img, ty, tx); }
