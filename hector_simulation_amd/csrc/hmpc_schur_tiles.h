// Tile grids of the matrix-core sweeps, and the index arithmetic of the block start's Schur tiles: everything here is plain
// integer C++ (no HIP type or builtin), so that it compiles for the device inside hmpc_kernel.h and on the host for
// tests/test_schur_tile_index.py, which checks it against the plain per-entry expressions it replaces.
//
//  (1) the deal of the NTG (NTG + 1) / 2 upper-triangle tiles of 16 x 16 to the waves (mfs_owner, MfsTiles): stage S and the
//      Schur inversion share it;
//  (2) where entry (i, j) of a Schur tile lies in the packed triangle of E, whether it is data or identity padding, and which
//      tiles of the grid hold no data at all -- from lane constants that are formed once per call (SchurLane) plus compile-time
//      constants, instead of a min / max, a compare and hi (hi + 1) / 2 + lo per entry.
#pragma once

#if defined(__HIPCC__)
#define HMPC_TILES_FN __host__ __device__ __forceinline__
#else
#define HMPC_TILES_FN inline
#endif

namespace hmpc {

// tile t (block-row-major over I <= J of the NTG x NTG grid of 16 x 16 tiles) -> I, J
constexpr int mfs_tile_i(int t, int ntg) {
  int i = 0, base = 0;
  while (t >= base + (ntg - i)) base += ntg - i, ++i;
  return i;
}
constexpr int mfs_tile_j(int t, int ntg) {
  int i = 0, base = 0;
  while (t >= base + (ntg - i)) base += ntg - i, ++i;
  return i + (t - base);
}
// Which wave holds tile (I, J).  By default the NTG (NTG + 1) / 2 tiles are dealt in contiguous runs of the block-row-major
// order (a wave then needs few distinct A operands: one per tile row it touches).  The 12 x 12 grid on four waves (180
// variables, two leg-step blocks per thread) is dealt by hand instead: there the 160 accumulator registers and the 144
// registers of the two blocks have to pass each other in the register file when M is handed over chunk by chunk
// (mfs_relayout), and what bounds the peak is how many of a wave's tiles are still unstored when its blocks are born -- a
// thread's slot-0 block lies in row chunk 0 (wave 3: 0-1), its slot-1 block in chunk 1 / 1-2 / 2-3 / 3 for waves 0..3.  With
// tiles per row chunk (9, 7, 4, 0), (8, 8, 4, 0), (8, 5, 3, 3), (8, 4, 4, 3) for waves 0..3 no wave holds more than 176 registers
// of matrix at any time (contiguous runs: 232, and the allocator spills); every wave owns three diagonal tiles.
constexpr int mfs_owner(int ntg, int nwv, int I, int J) {
  if (ntg == 12 && nwv == 4) {
    switch (I) {
      case 0: return J <= 8 ? 0 : 1;
      case 1: return J <= 5 ? 1 : 2;
      case 2: return J <= 3 ? 2 : 3;
      case 3: return J <= 9 ? 0 : 1;
      case 4: return J <= 9 ? 1 : 2;
      case 5: return J <= 7 ? 2 : 3;
      case 6: return J <= 9 ? 0 : 1;
      case 7: return J <= 8 ? 1 : 2;
      case 8: return 3;
      case 9: return 2;
      default: return 3;
    }
  }
  // 8 x 8 grid on four waves (120 variables): tile rows dealt in pairs I, 7 - I (8 + 1, 7 + 2, 6 + 3, 5 + 4 tiles): every wave
  // touches exactly two tile rows (two A operands per step instead of up to four) and owns two diagonal tiles
  if (ntg == 8 && nwv == 4) return I < 4 ? I : 7 - I;
  const int ntiles = ntg * (ntg + 1) / 2, base = ntiles / nwv, rem = ntiles % nwv;
  int t = 0;  // index of (I, J) in block-row-major order
  for (int i = 0; i < I; ++i) t += ntg - i;
  t += J - I;
  int w = 0, first = 0;
  while (w < nwv - 1 && t >= first + base + (w < rem ? 1 : 0)) first += base + (w < rem ? 1 : 0), ++w;
  return w;
}
constexpr int mfs_count(int ntg, int nwv, int wv) {
  int c = 0;
  for (int i = 0; i < ntg; ++i)
    for (int j = i; j < ntg; ++j) c += (mfs_owner(ntg, nwv, i, j) == wv) ? 1 : 0;
  return c;
}
template <int NTG, int NWV>
struct MfsGrid {
  static constexpr int NTILES = NTG * (NTG + 1) / 2;
  static constexpr int TPW = (NTILES + NWV - 1) / NWV;  // accumulator tiles per wave (some waves may hold one less)
};
template <int NTG, int NWV, int WV>
struct MfsTiles {  // the wave's tiles, sorted by (I, J)
  static constexpr int TPW = MfsGrid<NTG, NWV>::TPW;
  int cnt;
  int i[TPW], j[TPW];
  constexpr MfsTiles() : cnt(0), i{}, j{} {
    for (int ii = 0; ii < NTG; ++ii)
      for (int jj = ii; jj < NTG; ++jj)
        if (mfs_owner(NTG, NWV, ii, jj) == WV) i[cnt] = ii, j[cnt] = jj, ++cnt;
    for (int t = cnt; t < TPW; ++t) i[t] = i[cnt - 1], j[t] = j[cnt - 1];  // (a slot beyond the wave's count is never used)
  }
};
static_assert(mfs_count(12, 4, 0) == 20 && mfs_count(12, 4, 1) == 20 && mfs_count(12, 4, 2) == 19 && mfs_count(12, 4, 3) == 19, "12 x 12 deal");
static_assert(mfs_count(8, 4, 0) == 9 && mfs_count(8, 4, 3) == 9, "8 x 8 deal");

// ---- Schur tiles (schur_load / schur_store of hmpc_kernel.h) -----------------------------------------------------------------
// Lane (g, c) = (lane / 16, lane % 16) of a wave holds, in register r of tile (I, J), the entry of row i = 16 I + 4 r + g and
// column j = 16 J + c.  E is a packed lower triangle: entry (hi, lo), hi >= lo, at tri(hi) + lo.  With a = 16 I + 4 r and b = 16 J
// (compile-time constants)
//     tri(a + g) = tri(a) + a g + tri(g),      tri(b + c) = tri(b) + b c + tri(c)
// so tri(i) and tri(j) cost one multiply-add each on lane constants, tri(j) once per tile COLUMN.  In a tile above the diagonal
// tiles (J > I) i < j holds for every entry: the offset is tri(j) + i, a lane constant plus a compile-time constant, and the
// entry is data iff j < k0 (i < j).  Only the diagonal tiles compare: i <= j iff 4 r + g <= c.
constexpr int schur_tri(int i) { return i * (i + 1) / 2; }
struct SchurLane {
  int g, c;    // lane / 16, lane % 16
  int tg, tc;  // tri(g), tri(c)
};
HMPC_TILES_FN SchurLane schur_lane(const int lane) {
  const int g = lane >> 4, c = lane & 15;
  return SchurLane{g, c, schur_tri(g), schur_tri(c)};
}
// tri(j) of the lane's column in tile column J; tri(i) of its row r in tile row I
HMPC_TILES_FN int schur_col_tri(const SchurLane &L, const int J) { return schur_tri(16 * J) + 16 * J * L.c + L.tc; }
HMPC_TILES_FN int schur_row_tri(const SchurLane &L, const int I, const int r) { return schur_tri(16 * I + 4 * r) + (16 * I + 4 * r) * L.g + L.tg; }
// diagonal tiles: the entry lies on or above the diagonal (i <= j) / on it
HMPC_TILES_FN bool schur_upper(const SchurLane &L, const int r) { return 4 * r + L.g <= L.c; }
HMPC_TILES_FN bool schur_on_diagonal(const SchurLane &L, const int I, const int J, const int r) { return I == J && 4 * r + L.g == L.c; }
// offset of entry (i, j) of tile (I, J), I <= J, in the packed triangle; coltri = schur_col_tri(L, J), rowtri = schur_row_tri(L, I, r).
// The store writes the upper entries only (i <= j: schur_offset_upper); the load takes the lower half of a diagonal tile from the mirror.
HMPC_TILES_FN int schur_offset_upper(const SchurLane &L, const int I, const int r, const int coltri) { return coltri + (16 * I + 4 * r) + L.g; }
HMPC_TILES_FN int schur_offset(const SchurLane &L, const int I, const int J, const int r, const int coltri, const int rowtri) {
  if (I != J || schur_upper(L, r)) return schur_offset_upper(L, I, r, coltri);
  return rowtri + 16 * J + L.c;
}
// data or padding: the lane's column (once per tile column), its row (once per tile row and r), the entry
HMPC_TILES_FN bool schur_col_valid(const SchurLane &L, const int J, const int k0) { return 16 * J + L.c < k0; }
HMPC_TILES_FN bool schur_row_valid(const SchurLane &L, const int I, const int r, const int k0) { return 16 * I + 4 * r + L.g < k0; }
HMPC_TILES_FN bool schur_load_valid(const int I, const int J, const bool colv, const bool rowv) { return I == J ? (colv && rowv) : colv; }
HMPC_TILES_FN bool schur_store_valid(const SchurLane &L, const int I, const int J, const int r, const bool colv) {
  return I == J ? (colv && schur_upper(L, r)) : colv;
}
// power-of-two scaling exponent k = -floor(log2 S0_ii / 2) of a row or column from the high word of S0_ii > 0; 0 for padding
HMPC_TILES_FN int schur_exponent(const int diag_hi_word, const bool valid) {
  const int ex = ((diag_hi_word >> 20) & 2047) - 1023;
  return valid ? -(ex >> 1) : 0;
}
// A tile (I, J), I <= J, none of whose entries is data -- 16 J >= k0 -- is DEAD: identity padding from load to store.  Uniform over
// the workgroup; J live implies I live.  The ceil(k0 / 4) pivot steps end before the first dead tile row: no step pivots in one.
HMPC_TILES_FN bool schur_tile_live(const int J, const int k0) { return 16 * J < k0; }
HMPC_TILES_FN int schur_steps(const int k0) { return (k0 + 3) >> 2; }

}  // namespace hmpc
