// The 64 x 16 tile binning of libjxl_amd/csrc/tile_bins.h (what jxlhip_set_splines and jxlhip_set_patches upload for
// k_splines / k_patches) against a restatement that, for every tile, scans all rectangles.  A stand-alone program, built
// with -fsanitize=address,undefined by tests/test_tile_bins.py.  Prints "<lists checked> <most entries in one tile>".
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../libjxl_amd/csrc/tile_bins.h"

using jxlhip::TileBins;
using jxlhip::TileRect;

static long g_lists = 0;
static size_t g_most = 0;

#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      fprintf(stderr, "%s:%d: %s (frame %ux%u, %zu rectangles)\n", __FILE__, __LINE__, #cond, W, H, r.size()); \
      exit(1);                                                                             \
    }                                                                                      \
  } while (0)

static void Check(const std::vector<TileRect>& r, uint32_t W, uint32_t H) {
  TileBins b;
  b.words.assign(7, 0xDEADBEEFu);  // (whatever an earlier frame left)
  CHECK(jxlhip::BinTiles(r.data(), r.size(), W, H, &b));
  const uint32_t tx = (W + 63) / 64, ty = (H + 15) / 16, tiles = tx * ty;
  CHECK(b.tiles_x == tx && b.num_tiles == tiles);
  // the restatement: per tile, every rectangle that overlaps it, in record order
  std::vector<uint32_t> start(1, 0), idx, active;
  for (uint32_t t = 0; t < tiles; t++) {
    const uint32_t x0 = (t % tx) * 64, y0 = (t / tx) * 16;
    for (size_t i = 0; i < r.size(); i++)
      if (r[i].x0 < x0 + 64 && r[i].x1 > x0 && r[i].y0 < y0 + 16 && r[i].y1 > y0) idx.push_back((uint32_t)i);
    if (idx.size() != start.back()) active.push_back(t);
    if (idx.size() - start.back() > g_most) g_most = idx.size() - start.back();
    start.push_back((uint32_t)idx.size());
  }
  CHECK(b.entries == idx.size() && b.num_active == active.size());
  CHECK(b.words.size() == (size_t)tiles + 1 + b.entries + b.num_active);
  const uint32_t* tile_start = b.words.data();
  const uint32_t* tile_idx = tile_start + tiles + 1;
  const uint32_t* act = tile_idx + b.entries;
  CHECK(tile_start[0] == 0 && tile_start[tiles] == b.entries);
  for (uint32_t t = 0; t < tiles; t++) {
    CHECK(tile_start[t] <= tile_start[t + 1]);
    CHECK(tile_start[t + 1] == start[t + 1]);
    for (uint32_t k = tile_start[t]; k < tile_start[t + 1]; k++) {
      CHECK(k == tile_start[t] || tile_idx[k - 1] < tile_idx[k]);
      CHECK(tile_idx[k] == idx[k]);
    }
  }
  for (uint32_t a = 0; a < b.num_active; a++) {
    CHECK(act[a] == active[a]);
    CHECK(tile_start[act[a] + 1] > tile_start[act[a]] && (a == 0 || act[a - 1] < act[a]));
  }
  if (r.empty()) CHECK(b.entries == 0 && b.num_active == 0);
  g_lists++;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t Rand(uint32_t n) {  // [0, n), xorshift64*
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return (uint32_t)(((g_rng * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

int main() {
  static const uint32_t kSizes[6][2] = {{1, 1}, {63, 15}, {64, 16}, {65, 17}, {130, 33}, {200, 50}};
  for (const auto& s : kSizes) {
    const uint32_t W = s[0], H = s[1];
    // [x0, x1) x [y0, y1) clipped to the frame; dropped when nothing of it is inside
    auto clip = [&](uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, std::vector<TileRect>* out) {
      if (x1 > W) x1 = W;
      if (y1 > H) y1 = H;
      if (x0 < x1 && y0 < y1) out->push_back({x0, y0, x1, y1});
    };
    std::vector<TileRect> hand;
    Check(hand, W, H);  // the empty list
    clip(0, 0, 1, 1, &hand), clip(W - 1, 0, W, 1, &hand), clip(0, H - 1, 1, H, &hand), clip(W - 1, H - 1, W, H, &hand);
    clip(0, 0, W, H, &hand);                                   // the whole frame
    clip(10, 0, 64, 3, &hand), clip(64, 2, 70, 5, &hand);       // last column 63, first column 64
    clip(3, 4, 9, 16, &hand), clip(5, 16, 8, 20, &hand);        // last row 15, first row 16
    clip(60, 12, 68, 20, &hand);                               // across both edges
    clip((W - 1) / 64 * 64, (H - 1) / 16 * 16, W + 40, H + 40, &hand);  // the frame's last, partial tile
    clip(W - 1, 0, W + 100, H, &hand);
    Check(hand, W, H);
    for (size_t i = 0; i < hand.size(); i++) Check(std::vector<TileRect>(1, hand[i]), W, H);
    for (int it = 0; it < 500; it++) {
      std::vector<TileRect> r(Rand(301));
      const bool small = Rand(2) != 0;  // half the lists: rectangles of patch size, the others of any size
      for (TileRect& q : r) {
        q.x0 = Rand(W);
        q.y0 = Rand(H);
        q.x1 = q.x0 + 1 + Rand(small && W - q.x0 > 24 ? 24 : W - q.x0);
        q.y1 = q.y0 + 1 + Rand(small && H - q.y0 > 24 ? 24 : H - q.y0);
      }
      Check(r, W, H);
    }
  }
  printf("%ld %zu\n", g_lists, g_most);
  return 0;
}
