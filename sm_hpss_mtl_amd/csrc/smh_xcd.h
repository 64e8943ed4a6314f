// The per-XCD item list: a 1-D grid whose workgroups take the n items of a launch in 8 CONTIGUOUS ranges, one per XCD.
// Workgroup i of a grid is dispatched to XCD i % 8, each XCD with its own L2.  Where neighbouring items share memory, consecutive
// items on consecutive XCDs waste it.  The STFT is the measured case: a row of S is T frames (98: 392 bytes) and a tile writes an
// 80-byte piece of it, so the lines of a row are completed by up to three tiles -- in one L2 they merge before they leave for HBM;
// on the plain (tile, clip) grid every piece left as a partial line (WRITE_SIZE 105 MB for 80.7 MB of S), and the 240 samples that
// neighbouring tiles share were fetched twice.  So the items, in clip-major order, are cut into 8 ranges of ceil(n / 8): workgroup i
// takes item (i % 8) * ceil(n / 8) + i / 8, the grid is rounded up to a multiple of 8 and the workgroups past the list return.  The rule
// serves a thousand clips (an XCD owns 128 whole ones) and one long file (an eighth of its tiles) alike.  The host part needs no HIP.
#pragma once

namespace smh {
constexpr unsigned xcd_grid(long long n_items) { return (unsigned)(8 * ((n_items + 7) / 8)); }   // workgroups of the 1-D grid
constexpr bool xcd_fits(long long n_items) { return n_items < (1ll << 31) - 8; }  // the grid and the 32-bit decode below hold them
#ifdef __HIPCC__
// item n of this workgroup; false: none (a workgroup past the list)
__device__ __forceinline__ bool xcd_item(unsigned n_items, unsigned &n) {  // (n_items >= 0 below 2^31 - 8: xcd_fits)
    const unsigned per_xcd = (n_items + 7u) >> 3, j = blockIdx.x >> 3;
    n = (blockIdx.x & 7u) * per_xcd + j;
    return j < per_xcd && n < n_items;
}
#endif
}  // namespace smh
