// tile_bins.h -- the 64 x 16 tile binning k_splines and k_patches read (kernels_splines.hip, kernels_patches.hip).
// Host only, nothing of HIP: render_stages.hip and the harness of tests/fuzz/ build it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace jxlhip {

struct TileRect { uint32_t x0, y0, x1, y1; };  // [x0, x1) x [y0, y1): not empty, inside the frame

// words = tile_start (num_tiles + 1: tile t's entries are tile_idx[tile_start[t] .. tile_start[t + 1])), tile_idx
// (`entries` record indices, increasing within a tile), active (the num_active tiles with entries, increasing)
struct TileBins {
  std::vector<uint32_t> words;
  uint32_t tiles_x = 0, num_tiles = 0, num_active = 0;
  size_t entries = 0;
};

// Bins the n rectangles (in record order) of a W x H frame.  false: the list does not fit 32-bit offsets -- refused
// before anything is sized by it, and *b is not to be used.
inline bool BinTiles(const TileRect* r, size_t n, uint32_t W, uint32_t H, TileBins* b) {
  const uint32_t tx = (W + 63) / 64, ty = (H + 15) / 16, tiles = tx * ty;
  std::vector<uint32_t> count(tiles, 0);  // per tile: its entries, then its write cursor
  for (size_t i = 0; i < n; i++)
    for (uint32_t y = r[i].y0 / 16; y <= (r[i].y1 - 1) / 16; y++)
      for (uint32_t x = r[i].x0 / 64; x <= (r[i].x1 - 1) / 64; x++) count[y * tx + x]++;
  std::vector<uint32_t>& w = b->words;
  w.assign(tiles + 1, 0);
  uint32_t active = 0;
  uint64_t total = 0;
  for (uint32_t t = 0; t < tiles; t++) {
    active += count[t] != 0;
    total += count[t];
    w[t + 1] = (uint32_t)total;
  }
  b->tiles_x = tx;
  b->num_tiles = tiles;
  b->num_active = active;
  b->entries = (size_t)total;
  if (total > 0xFFFFFFFFull - tiles - active - 1) return false;
  w.resize(tiles + 1 + b->entries + active);
  for (uint32_t t = 0; t < tiles; t++) count[t] = w[t];
  for (size_t i = 0; i < n; i++)
    for (uint32_t y = r[i].y0 / 16; y <= (r[i].y1 - 1) / 16; y++)
      for (uint32_t x = r[i].x0 / 64; x <= (r[i].x1 - 1) / 64; x++) w[tiles + 1 + count[y * tx + x]++] = (uint32_t)i;
  for (uint32_t t = 0, a = 0; t < tiles; t++)
    if (w[t + 1] != w[t]) w[tiles + 1 + b->entries + a++] = t;
  return true;
}

}  // namespace jxlhip
