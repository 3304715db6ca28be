// mrbo_lane_tables.h -- which entry of a packed triangle, and which (row, column) of the fantasy
// rows' gradient block, an index t owns: one 32-bit word per t, kept per wave in the lane-uniform
// LDS area (Lay::U_TAB, written once by wave_setup) and read where evaluate used to unrank t with a
// dependent compare / select chain in every evaluation.
//
// tri_unrank is that chain, as one constexpr function: wave_setup fills the table with it at run
// time, and LaneTables<D, FMAX> checks at compile time, for every t of every table, that the word
// made from it unpacks to the pair whose rank is t.  No device code here: the header also compiles
// alone with the host compiler (tests/test_lane_tables.py does that for every D and both FMAX).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MRBO_LT_FN __host__ __device__ constexpr
#else
#define MRBO_LT_FN constexpr
#endif

namespace mrbo {

struct TriPair { int a, b; };

// entry t of the row-major upper triangle (a ≤ b) of an n × n matrix
MRBO_LT_FN TriPair tri_unrank(int n, int t) {
  int a = 0, rem = t;
  for (int aa = 0; aa < n; ++aa) if (a == aa && rem >= n - aa) { rem -= n - aa; a = aa + 1; }
  return {a, a + rem};
}
// its inverse in closed form: rows 0..a-1 hold n, n-1, … entries
MRBO_LT_FN int tri_rank(int n, int a, int b) { return a * n - a * (a - 1) / 2 + (b - a); }

// Word t: Gram pair (a, b) of the (D+1)² triangle in bits 0-4 / 5-9, Hessian pair of the D²
// triangle in bits 10-14 / 15-19, phase 4b's row r = t / D in bits 20-22 and its column
// c = 1 + t % D in bits 23-27.  A field whose table is shorter than t holds 0.
struct LaneWord {
  enum { GA = 0, GB = 5, HA = 10, HB = 15, R = 20, C = 23, W5 = 31, W3 = 7 };
};
MRBO_LT_FN unsigned lane_field(unsigned w, int shift, unsigned mask) { return (w >> shift) & mask; }

// sizes of the three index ranges and of the table that holds them
template <int D, int FMAX>
struct LaneTableSize {
  static constexpr int D1 = D + 1;
  static constexpr int NG = D1 * (D1 + 1) / 2, NH = D * (D + 1) / 2, NYF = FMAX * D;
  static constexpr int NT = NG > NYF ? NG : NYF;   // NH < NG
  static_assert(D >= 1 && D1 <= 31 && FMAX <= 7 && NH < NG, "lane word: field widths");
};

template <int D, int FMAX>
MRBO_LT_FN unsigned lane_word(int t) {
  using Z = LaneTableSize<D, FMAX>;
  unsigned w = 0;
  if (t < Z::NG) {
    const TriPair g = tri_unrank(Z::D1, t);
    w |= (unsigned)g.a << LaneWord::GA | (unsigned)g.b << LaneWord::GB;
  }
  if (t < Z::NH) {
    const TriPair h = tri_unrank(D, t);
    w |= (unsigned)h.a << LaneWord::HA | (unsigned)h.b << LaneWord::HB;
  }
  if (t < Z::NYF) w |= (unsigned)(t / D) << LaneWord::R | (unsigned)(1 + t % D) << LaneWord::C;
  return w;
}

// word t unpacks to the pairs whose rank is t (so also: in range, a ≤ b, no field overflow)
template <int D, int FMAX>
MRBO_LT_FN bool lane_word_ok(int t) {
  using Z = LaneTableSize<D, FMAX>;
  const unsigned w = lane_word<D, FMAX>(t);
  const int ga = lane_field(w, LaneWord::GA, LaneWord::W5), gb = lane_field(w, LaneWord::GB, LaneWord::W5);
  const int ha = lane_field(w, LaneWord::HA, LaneWord::W5), hb = lane_field(w, LaneWord::HB, LaneWord::W5);
  const int r = lane_field(w, LaneWord::R, LaneWord::W3), c = lane_field(w, LaneWord::C, LaneWord::W5);
  if (t < Z::NG && !(ga <= gb && gb < Z::D1 && tri_rank(Z::D1, ga, gb) == t)) return false;
  if (t < Z::NH && !(ha <= hb && hb < D && tri_rank(D, ha, hb) == t)) return false;
  if (t < Z::NYF && !(r < FMAX && c >= 1 && c <= D && r * D + (c - 1) == t)) return false;
  return true;
}
template <int D, int FMAX>
MRBO_LT_FN bool lane_words_ok() {
  for (int t = 0; t < LaneTableSize<D, FMAX>::NT; ++t) if (!lane_word_ok<D, FMAX>(t)) return false;
  return true;
}

template <int D, int FMAX>
struct LaneTables : LaneTableSize<D, FMAX> {
  static constexpr int DOUBLES = (LaneTableSize<D, FMAX>::NT + 1) / 2;   // LDS footprint, in doubles
  static_assert(lane_words_ok<D, FMAX>(), "lane index table: a word does not unpack to the entry of its index");
};

}  // namespace mrbo
