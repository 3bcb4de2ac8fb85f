// Halo-tile conv instantiations for STRIDED forward convs (the discriminator's (4,4,k) stride (2,2,1|2)
// down-sampling layers, torch_blocks.py:138-142): 256-voxel output tiles - the input halo of a stride-2
// tile is 4..8x its output volume - as 8 waves x 2 m-tiles.
#include "conv_tile_impl.h"

template <int TPK>
static int run(CtArgs& a, hipStream_t st) {
  const int N = a.Cout;
  if (a.mask_y || a.ups) return WSR_EUNSUPPORTED;
  if constexpr (TPK == 2) {
    // the halo of a strided tile grows with the stride and the filter extent: fall back to flatter tiles
    // until the image fits the per-wave DMA budget and LDS.
    // With filters of <= 8 per axis and <= 125 taps (conv_geom_ok) and strides <= 2, {4,4,8} has a halo of at most
    // 14 x 14 x 15 = 2 940 voxels (8x8x1 taps): 92 of the 104 DMA units, and 92 KB of LDS that leave >= 4 K-steps of
    // weights at every width - launch_ct can only turn it away on its 32-bit offset test (the halo's x-planes hold
    // >= 2^32 elements), which depends on TX alone, or on the range test of the workgroup index.  {2,4,8} halves TX for
    // the former.  Its own halo (<= 10 x 14 x 22 = 3 080 voxels, 97 units) fits as well, so only those two tests can
    // refuse it, and a {2,2,8} after it - the same TX, more tiles, the same channel-group width wherever the tile
    // count matters - would fail them too: there is no fifth shape.
    static const int shapes[][3] = {{4, 4, 16}, {4, 8, 8}, {4, 4, 8}, {2, 4, 8}};
    for (const auto& sh : shapes) {
      a.TX = sh[0]; a.TY = sh[1]; a.TZ = sh[2] < a.Zo ? sh[2] : a.Zo;
      int rc;
      // few output tiles (the deep layers: 16x16x64 .. 4x4x32 voxels): narrower channel groups, more workgroups
      const long tiles = (long)a.B * ((a.Xo + a.TX - 1) / a.TX) * ((a.Yo + a.TY - 1) / a.TY) * ((a.Zo + a.TZ - 1) / a.TZ);
      const bool few = !WSR_ENV_SET("WSR_CT_STRIDED_WIDE") && tiles * ((N + 127) / 128) < 128;
      if (N <= 32 || (few && tiles * ((N + 63) / 64) < 128)) rc = launch_ct<8, 1, 2, 2, TPK>(a, st);
      else if (N <= 64 || few) rc = launch_ct<8, 1, 2, 4, TPK>(a, st);
      else rc = launch_ct<8, 1, 2, 8, TPK>(a, st);  // wider outputs: groups of 128 channels
      if (rc != WSR_EUNSUPPORTED) return rc;
    }
  }
  return WSR_EUNSUPPORTED;
}

int wsr_ct_run_strided(CtArgs& a, int tpk, hipStream_t st) {
  if (tpk == 2) return run<2>(a, st);
  return WSR_EUNSUPPORTED;
}
