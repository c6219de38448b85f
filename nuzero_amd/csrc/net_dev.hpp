// Fused policy/value network for one tile of 16 positions (gfx950 matrix cores).
// Device function shared by the stand-alone network kernel (net.hip) and the
// persistent self-play kernel (selfplay.hip).
//
// Computes Network_Manager.inference (Neural_Networks/Network_Manager.py:46-64)
// for the square-conv RecurrentNet / ResNet / ConvNet (Neural_Networks/Architectures/
// RecurrentNet.py:82-99; BasicBlock blocks.py:37-41; Reduce_PolicyHead
// blocks.py:130-170; Reduce_ValueHead blocks.py:46-92) on a batch of 3x3 boards:
// every conv is 3x3, stride 1, zero 'same' padding, bias-free.
//
// One workgroup runs the WHOLE network for 16 positions; activations never
// leave LDS and the weights stream from L2 straight into registers.
//
// Mapping.  On a 3x3 board with a 3x3 kernel every output cell o sees input
// cell i through exactly one tap (tap = i - o + centre) when |dy|,|dx| <= 1, so
// a conv layer is, per output cell, a dense [C_out] x [C_in * n_valid(o)] x
// [16 positions] product.  The zero-padding taps are never multiplied: 49 of the 81
// (cell, tap) pairs exist.
//
// Arithmetic.  Every float32 product a * w is formed on the BF16 matrix cores from exact
// three-way splits a = a0 + a1 + a2, w = w0 + w1 + w2 (each piece the next 8 significant
// bits, a bf16 number) as the six terms a1w1 + a2w0 + a0w2 + a1w0 + a0w1 + a0w0 accumulated
// in float32; the dropped terms are below 2^-23 |a w|, the rounding of the float32 product
// itself.  v_mfma_f32_16x16x32_bf16 runs at 16x the FP32 MFMA rate, so the six of them per
// 32 channels take 96 cycles where eight v_mfma_f32_16x16x4_f32 take 256.  Measured against
// float64-accumulated convolutions the result is closer than a plain float32 convolution
// (DESIGN.md section 4).  The weights are split once on the host (engine.hip pack_conv), the
// activations once per element in the epilogue that produces them: LDS holds the three bf16
// pieces, the K loop reads them and issues MFMAs, nothing else.  The (<= 4) raw input planes of
// the projection / recall convs go through one v_mfma_f32_16x16x4_f32 per pair.
// That is the default mode, PREC_F32.  The opt-in plain-bf16 mode (PREC_BF16, nz_engine_precision; the rule is stated once,
// in fused16_dev.hpp) keeps ONE rounded bf16 per weight and stored activation -- piece plane 0 of the same layout -- and
// issues one MFMA per pair and K group; see PiecesT below.  It exists for the 16-column pass on a wave's own job list.
//
// Orientation.  The weights are the MFMA's A operand (rows = 16 output channels), the
// activations its B operand (columns = 16 positions): lane l supplies W[cout = l & 15]
// [k = 8 (l >> 4) + j] and X[k = 8 (l >> 4) + j][pos = l & 15], j = 0..7, and receives
// C[cout = 4 (l >> 4) + r][pos = l & 15] in register r -- four consecutive channels of one
// position, which the epilogue splits and writes as one 8-byte LDS store per piece.  Each
// position's column is independent of the others, so a position's outputs do not depend on
// which batch slot it occupies.
//
// Work split.  The host compiles the network into one job list per wave
// (engine.hip): a job is one (layer, 16-channel output tile, output-cell group).
// 64-channel layers give each of the 4 waves one full tile; the narrow head layers are cut
// by output-cell group as well so that all four matrix pipes stay busy.  Per 32-channel K
// group a wave reads 3 x 16 bytes per used input cell from LDS (refilled in place for the next
// K group as soon as the last tap that needs a cell has issued) and streams the weights tap by
// tap from L2, one whole K group ahead of the MFMAs -- also across jobs and stage barriers.
//
// LDS layout: act[buffer][piece][cell][pos][64 ch] bf16, the 16-byte slot index XOR-ed with
// (pos >> 1) & 7 so that ds_read_b128 (operands) and ds_write_b64 (epilogue) are
// bank-conflict free.  Two buffers (ping-pong; residual blocks update in place), and a 16-channel strip
// strip[piece][cell][pos][16 ch] (16-byte slot index XOR-ed with (pos >> 2) & 1) for the one head tile that finds no
// room in them: the two heads' first convs run as one stage, and their 48 + 32 output channels exceed one buffer's 64.
#pragma once
#include <type_traits>

#include "bf16_split.hpp"
#include "engine.h"

namespace nz {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int POS = 16;            // positions per workgroup (MFMA N)
constexpr int CELLS = 9;
constexpr int ROW = 64;            // channels per (cell, pos) row
constexpr int NET_WAVES = 8;            // two wavefronts per SIMD: one's epilogue / operand loads run under the other's MFMAs
constexpr int NET_THREADS = NET_WAVES * 64;
constexpr int NET_BUFFERS = NET_ACT_BUFFERS;
constexpr int PIECE_BYTES = CELLS * POS * ROW * 2;          // one bf16 piece of one buffer
constexpr int ACT_BYTES = 3 * PIECE_BYTES;
constexpr int ACT_FLOATS = ACT_BYTES / 4;                   // LDS is declared as float[] by the kernels
constexpr int INP_FLOATS = CELLS * POS * 4;
constexpr int VAL_FLOATS = CELLS * POS;                      // the value head's last layer, per cell, before the mean
constexpr int STRIP_PIECE_BYTES = CELLS * POS * 16 * 2;     // one bf16 piece of the strip: a quarter of a buffer's piece
constexpr int STRIP_FLOATS = 3 * STRIP_PIECE_BYTES / 4;
constexpr int NET_LDS_FLOATS = NET_BUFFERS * ACT_FLOATS + INP_FLOATS + VAL_FLOATS + STRIP_FLOATS;
constexpr int TAP_DWORDS = 3 * 64 * 4;                      // one tap of one K group: [piece][lane][8 bf16]
constexpr int W_RING = 3;                                   // taps in flight: the weight stream runs three taps ahead of the MFMAs
// the same of the plain-bf16 stream (PREC_BF16; bf16_split.hpp): no piece dimension, [lane][8 bf16] a tap
constexpr int tap_dwords(int prec) { return prec_pieces(prec) * 64 * 4; }
constexpr int kg_dwords(int prec) { return 9 * tap_dwords(prec); }
static_assert(tap_dwords(PREC_F32) == TAP_DWORDS && kg_dwords(PREC_BF16) == NET_KG_DWORDS_BF16, "host packing and kernel agree");
static_assert(NET_WAVES == NET_WAVES_HOST, "job lists are per wave");
static_assert(NET_KG_DWORDS == 9 * TAP_DWORDS && NET_KG_CHANNELS == 32, "host packing (engine.hip) and kernel agree");

// output-cell groups: all nine | four quarters {4,0} {1,3} {5,7} {2,6,8} | two halves {0,1,2,3,5} {4,6,7,8}
// ((input cell, tap) pairs: 49 | 13, 12, 12, 12 | 26, 23).  The halves of a tile go to the two waves of a SIMD: the older
// wave wins the matrix pipe, so its epilogue runs under the other's MFMAs and one epilogue is left when those end.
// (An uneven 7 + 2 split leaves a shorter epilogue but measured the same and spilled four registers in the large job.)
// (og_mask: engine.h)

// byte offset of the 16-byte slot holding channels 8 s .. 8 s + 7 of (cell, pos) inside one piece
__device__ __forceinline__ int slot_addr(int cell, int pos, int s) {
  return ((cell * POS + pos) << 7) + (((s ^ (pos >> 1)) & 7) << 4);
}
// the same inside one piece of the strip (s = 0, 1): every stride is a quarter of the buffer's
__device__ __forceinline__ int strip_addr(int cell, int pos, int s) {
  return ((cell * POS + pos) << 5) + (((s ^ (pos >> 2)) & 1) << 4);
}

template <int I, int TAP>
struct TapMap {   // output cell reached from input cell I through tap TAP
  static constexpr int dy = TAP / 3 - 1, dx = TAP % 3 - 1;
  static constexpr int oy = I / 3 - dy, ox = I % 3 - dx;
  static constexpr bool valid = oy >= 0 && oy < 3 && ox >= 0 && ox < 3;
  static constexpr int o = valid ? oy * 3 + ox : 0;
};
template <int OMASK, int I, int TAP>
constexpr bool pair_used() { return TapMap<I, TAP>::valid && ((OMASK >> TapMap<I, TAP>::o) & 1); }
template <int OMASK, int I>
constexpr bool input_used() {
  return pair_used<OMASK, I, 0>() || pair_used<OMASK, I, 1>() || pair_used<OMASK, I, 2>() ||
         pair_used<OMASK, I, 3>() || pair_used<OMASK, I, 4>() || pair_used<OMASK, I, 5>() ||
         pair_used<OMASK, I, 6>() || pair_used<OMASK, I, 7>() || pair_used<OMASK, I, 8>();
}

// first / last tap (0..8) that reads input cell I for this output-cell group
template <int OMASK, int I>
constexpr int first_use() {
  return pair_used<OMASK, I, 0>() ? 0 : pair_used<OMASK, I, 1>() ? 1 : pair_used<OMASK, I, 2>() ? 2 :
         pair_used<OMASK, I, 3>() ? 3 : pair_used<OMASK, I, 4>() ? 4 : pair_used<OMASK, I, 5>() ? 5 :
         pair_used<OMASK, I, 6>() ? 6 : pair_used<OMASK, I, 7>() ? 7 : 8;
}
template <int OMASK, int I>
constexpr int last_use() {
  return pair_used<OMASK, I, 8>() ? 8 : pair_used<OMASK, I, 7>() ? 7 : pair_used<OMASK, I, 6>() ? 6 :
         pair_used<OMASK, I, 5>() ? 5 : pair_used<OMASK, I, 4>() ? 4 : pair_used<OMASK, I, 3>() ? 3 :
         pair_used<OMASK, I, 2>() ? 2 : pair_used<OMASK, I, 1>() ? 1 : 0;
}
// last valid tap of output cell O (engine.h net_final_tap): in the tap-major K loop the cell's accumulator is final once
// that tap of the job's last K group has issued -- cell 8 after tap 4, cells 6, 7 after tap 5, cells 2, 5 after tap 7
template <int OMASK, int O>
constexpr int final_tap() {
  static_assert((OMASK >> O) & 1, "cell of the job's group");
  return net_final_tap(O);
}
static_assert(net_final_tap(8) == 4 && net_final_tap(6) == 5 && net_final_tap(7) == 5 && net_final_tap(2) == 7 &&
              net_final_tap(5) == 7 && net_final_tap(0) == 8 && net_final_tap(1) == 8 && net_final_tap(3) == 8 &&
              net_final_tap(4) == 8, "tap = 3 (dy + 1) + (dx + 1), input cell = output cell + (dy, dx)");
// (input cell, tap) pairs of the group that issue before pair (I, TAP) in a K group (tap-major, input cells ascending);
// pairs_before(omask, 9, 0): all of them
constexpr int pairs_before(int omask, int tap, int i) {
  int n = 0;
  for (int t = 0; t < 9; ++t)
    for (int c = 0; c < CELLS; ++c) {
      const int oy = c / 3 - (t / 3 - 1), ox = c % 3 - (t % 3 - 1);
      const bool used = oy >= 0 && oy < 3 && ox >= 0 && ox < 3 && ((omask >> (oy * 3 + ox)) & 1);
      if (used && (t < tap || (t == tap && c < i))) ++n;
    }
  return n;
}
static_assert(pairs_before(0x1FF, 9, 0) == 49 && pairs_before(0x02F, 9, 0) == 26 && pairs_before(0x1D0, 9, 0) == 23, "og_mask");
// The group's early cells -- final before tap 8 -- in the order they become final (then by index): how many, and the
// qi-th of them (-1: none)
constexpr int early_cell(int omask, int qi) {
  for (int t = 0; t < 8; ++t)
    for (int o = 0; o < CELLS; ++o)
      if (((omask >> o) & 1) && net_final_tap(o) == t && qi-- == 0) return o;
  return -1;
}
constexpr int early_cells(int omask) {
  int n = 0;
  while (early_cell(omask, n) >= 0) ++n;
  return n;
}

// When cell I's operands of the SECOND K group are read, on a timeline of 18 steps (step s < 9: after tap s of the first
// K group; step 9 + t: before tap t of the second): not before the first group is done with the registers, and not
// earlier than REFILL_AHEAD taps before the second group needs them -- operands that sit in registers for a whole K
// group cost the large jobs their last free registers (a four-register spill around the K loop otherwise).
constexpr int REFILL_AHEAD = 3;
template <int OMASK, int I>
constexpr int refill_step() {
  constexpr int earliest = last_use<OMASK, I>();                       // after that tap of group one
  constexpr int wanted = 9 + first_use<OMASK, I>() - REFILL_AHEAD;      // before that tap of group two
  return wanted > earliest ? wanted : earliest;
}

// PREC (PREC_F32 / PREC_BF16, bf16_split.hpp) is a template parameter of everything that holds or multiplies operands;
// the float32 mode is the default and what the names without it mean.  Plain-bf16 mode: ONE rounded bf16 per weight and
// stored activation (piece plane 0 of the same LDS layout; planes 1 and 2 are neither written nor read), one MFMA per
// (input cell, tap) pair and K group in the same order, the same float32 accumulator and activation functions, the
// residual added as the stored bf16 value, end-of-job epilogues only, no whole-tile job (the rule: fused16_dev.hpp).
template <int PREC>
struct PiecesT {          // the bf16 pieces (three; PREC_BF16: one) of 8 channels (one lane's share of a 32-channel K group)
  u32x4 p[prec_pieces(PREC)];
};
template <int PREC>
struct FragST {           // the wavefront's weight stream, W_RING taps ahead of the MFMAs
  PiecesT<PREC> rb[W_RING];
};
typedef PiecesT<PREC_F32> Pieces;
typedef FragST<PREC_F32> FragS;

// A job's activation operands of one K group.  Every group but the whole tile keeps the three pieces of each used input
// cell in registers for the K group.  The whole-tile job (0x1FF; solo lists only) holds all nine cells and all nine
// accumulators, and a third resident piece would not fit the register file beside the weight ring: piece 2, which
// only one of a pair's six MFMAs reads, is fetched from LDS per (input cell, tap) pair instead, LATE_AHEAD pairs ahead
// into a ring of as many registers -- the same bits from the same address, 49 reads a K group in place of nine.
constexpr int resident_pieces(int omask, int prec = PREC_F32) { return prec == PREC_BF16 ? 1 : omask == 0x1FF ? 2 : 3; }
constexpr int LATE_AHEAD = 2;
// the n-th (input cell, tap) pair of the group in issue order, as 9 * tap + cell (-1: past the last)
constexpr int nth_pair(int omask, int n) {
  for (int t = 0; t < 9; ++t)
    for (int c = 0; c < CELLS; ++c) {
      const int oy = c / 3 - (t / 3 - 1), ox = c % 3 - (t % 3 - 1);
      if (oy >= 0 && oy < 3 && ox >= 0 && ox < 3 && ((omask >> (oy * 3 + ox)) & 1) && n-- == 0) return 9 * t + c;
    }
  return -1;
}
template <int OMASK, int PREC = PREC_F32>
struct Operands {
  static_assert(PREC == PREC_F32 || OMASK != 0x1FF, "no whole-tile job in plain-bf16 mode");
  static constexpr int NP = resident_pieces(OMASK, PREC), PAIRS = pairs_before(OMASK, 9, 0);
  PiecesT<PREC> x[CELLS];
  // NP == 2 only: the ring of piece 2, the source buffer, the slot addresses of this K group and of the job's next
  u32x4 late[LATE_AHEAD];
  const unsigned char* src;
  int cur, nxt;
  // pairs are counted through the job: pair N of the second K group (PART 2) is PAIRS + N
  template <int PART>
  static constexpr int through(int n) { return n + (PART == 2 ? PAIRS : 0); }
  template <int I, int N, int PART>
  __device__ __forceinline__ const u32x4& third() const {
    if constexpr (NP == 3) return x[I].p[2];
    else return late[through<PART>(N) % LATE_AHEAD];
  }
  // piece 2 for pair N of this K group, or (N >= PAIRS, PART 1) for pair N - PAIRS of the next; nothing past the job's end
  template <int N, int PART>
  __device__ __forceinline__ void fetch_third() {
    if constexpr (NP == 2 && (N < PAIRS || PART == 1)) {
      constexpr int I = nth_pair(OMASK, N % PAIRS) % 9;
      late[through<PART>(N) % LATE_AHEAD] =
          *reinterpret_cast<const u32x4*>(src + 2 * PIECE_BYTES + I * (POS * 128) + (N < PAIRS ? cur : nxt));
    }
  }
};

// ---- exact three-way split of float32 into bf16 pieces (the primitives: bf16_split.hpp) ----------------
// x = p0 + p1 + p2 exactly, 8 significant bits each
__device__ __forceinline__ void split_pair(float x0, float x1, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
  p0 = pack_hi16(x0, x1);
  const float r0 = x0 - bf16_trunc(x0);
  const float r1 = x1 - bf16_trunc(x1);
  p1 = pack_hi16(r0, r1);
  const float s0 = r0 - bf16_trunc(r0);
  const float s1 = r1 - bf16_trunc(r1);
  p2 = pack_hi16(s0, s1);
}
// The K loop's MFMAs carry slots: slot g follows the g-th MFMA of a K group (in issue order) and runs whatever the
// epilogue scheduler `e` has placed there (ProgEpi below; NoEpi: nothing, the chain is as before).
struct NoEpi {
  template <int G>
  __device__ __forceinline__ void slot(const f32x4 (&)[CELLS]) {}
};
template <int OMASK, int I, int TAP, int PART, typename E, int PREC>
__device__ __forceinline__ void pair_mfma(f32x4 (&acc)[CELLS], Operands<OMASK, PREC>& xs, const PiecesT<PREC>& w, E& e) {
  if constexpr (PREC == PREC_BF16) {             // the one product term; the pairs of a tap are independent accumulators
    if constexpr (pair_used<OMASK, I, TAP>()) {
      constexpr int o = TapMap<I, TAP>::o;
      acc[o] = mfma_bf16(w.p[0], xs.x[I].p[0], acc[o]);
    }
  } else if constexpr (pair_used<OMASK, I, TAP>()) {
    constexpr int o = TapMap<I, TAP>::o;
    constexpr int n = pairs_before(OMASK, TAP, I), g = 6 * n;
    const Pieces (&x)[CELLS] = xs.x;
    // small terms first; one accumulator chain issues at the full rate
    acc[o] = mfma_bf16(w.p[1], x[I].p[1], acc[o]); e.template slot<g + 0>(acc);
    acc[o] = mfma_bf16(w.p[0], xs.template third<I, n, PART>(), acc[o]); e.template slot<g + 1>(acc);
    acc[o] = mfma_bf16(w.p[2], x[I].p[0], acc[o]); e.template slot<g + 2>(acc);
    acc[o] = mfma_bf16(w.p[0], x[I].p[1], acc[o]); e.template slot<g + 3>(acc);
    acc[o] = mfma_bf16(w.p[1], x[I].p[0], acc[o]); e.template slot<g + 4>(acc);
    acc[o] = mfma_bf16(w.p[0], x[I].p[0], acc[o]); e.template slot<g + 5>(acc);
    xs.template fetch_third<n + LATE_AHEAD, PART>();      // (whole-tile job only) into the register this pair just read
    // keep the chain together: the scheduler would interleave it with the other pairs' chains, and
    // round-robin over accumulators issues at 21 cycles per MFMA instead of 16
    // (scripts/microbench/mfma_bf16_rate.hip)
    __builtin_amdgcn_sched_barrier(0);
  }
}
// all (input cell, TAP) pairs of the job's output cells: independent accumulators
template <int OMASK, int TAP, int PART, typename E, int PREC>
__device__ __forceinline__ void tap_mfma(f32x4 (&acc)[CELLS], Operands<OMASK, PREC>& xs, const PiecesT<PREC>& w, E& e) {
  pair_mfma<OMASK, 0, TAP, PART>(acc, xs, w, e); pair_mfma<OMASK, 1, TAP, PART>(acc, xs, w, e); pair_mfma<OMASK, 2, TAP, PART>(acc, xs, w, e);
  pair_mfma<OMASK, 3, TAP, PART>(acc, xs, w, e); pair_mfma<OMASK, 4, TAP, PART>(acc, xs, w, e); pair_mfma<OMASK, 5, TAP, PART>(acc, xs, w, e);
  pair_mfma<OMASK, 6, TAP, PART>(acc, xs, w, e); pair_mfma<OMASK, 7, TAP, PART>(acc, xs, w, e); pair_mfma<OMASK, 8, TAP, PART>(acc, xs, w, e);
  if constexpr (PREC == PREC_BF16) __builtin_amdgcn_sched_barrier(0);   // a tap's MFMAs stay together, ahead of the ring's refill
}

template <int OMASK, int I, int PREC>
__device__ __forceinline__ void load_cell(PiecesT<PREC> (&x)[CELLS], const unsigned char* __restrict__ src, int a0) {
#ifdef NZ_ABLATE_A   // timing-only build: no LDS reads of the activation operands (outputs are wrong)
  if constexpr (input_used<OMASK, I>()) {
    const uint32_t v = 0x3C003C00u + a0 + I;
#pragma unroll
    for (int piece = 0; piece < prec_pieces(PREC); ++piece) x[I].p[piece] = u32x4{v, v, v, v};
    asm volatile("" :: "v"(src));
  }
#else
  if constexpr (input_used<OMASK, I>()) {
#pragma unroll
    for (int piece = 0; piece < resident_pieces(OMASK, PREC); ++piece)
      x[I].p[piece] = *reinterpret_cast<const u32x4*>(src + piece * PIECE_BYTES + I * (POS * 128) + a0);
  }
#endif
}
// this lane's activation operands of one K group (slot address a0) for every used input cell
template <int OMASK, int PREC>
__device__ __forceinline__ void load_cells(PiecesT<PREC> (&x)[CELLS], const unsigned char* __restrict__ src, int a0) {
  load_cell<OMASK, 0>(x, src, a0); load_cell<OMASK, 1>(x, src, a0); load_cell<OMASK, 2>(x, src, a0);
  load_cell<OMASK, 3>(x, src, a0); load_cell<OMASK, 4>(x, src, a0); load_cell<OMASK, 5>(x, src, a0);
  load_cell<OMASK, 6>(x, src, a0); load_cell<OMASK, 7>(x, src, a0); load_cell<OMASK, 8>(x, src, a0);
}
// A K group split over two areas (NET_SSLOT_SPLIT): quads 0-1 read slots 6-7 of `src`, quads 2-3 slots 0-1 of the strip.
// The strip's strides are the buffer's shifted right by two, so one per-lane base and shift address both: the lanes
// supply the same channels as from one buffer, and the MFMAs see the same operands.
template <int OMASK, int I, int PREC>
__device__ __forceinline__ void load_cell_split(PiecesT<PREC> (&x)[CELLS], const unsigned char* base, unsigned sh) {
  if constexpr (input_used<OMASK, I>()) {
#pragma unroll
    for (int piece = 0; piece < prec_pieces(PREC); ++piece)
      x[I].p[piece] = *reinterpret_cast<const u32x4*>(base + ((unsigned)(piece * STRIP_PIECE_BYTES + I * (POS * 32)) << sh));
  }
}
template <int OMASK, int PREC>
__device__ __forceinline__ void load_cells_split(PiecesT<PREC> (&x)[CELLS], const unsigned char* __restrict__ src,
                                                 const unsigned char* __restrict__ strip, int pos, int quad) {
  const bool in_src = quad < 2;
  const unsigned char* base = in_src ? src + slot_addr(0, pos, 6 + quad) : strip + strip_addr(0, pos, quad - 2);
  const unsigned sh = in_src ? 2u : 0u;
  load_cell_split<OMASK, 0>(x, base, sh); load_cell_split<OMASK, 1>(x, base, sh); load_cell_split<OMASK, 2>(x, base, sh);
  load_cell_split<OMASK, 3>(x, base, sh); load_cell_split<OMASK, 4>(x, base, sh); load_cell_split<OMASK, 5>(x, base, sh);
  load_cell_split<OMASK, 6>(x, base, sh); load_cell_split<OMASK, 7>(x, base, sh); load_cell_split<OMASK, 8>(x, base, sh);
}
template <int PREC>
__device__ __forceinline__ void load_tap(PiecesT<PREC>& t, const float* __restrict__ w, int lane) {
#ifdef NZ_ABLATE_B   // timing-only build: no global loads of the weight operands (outputs are wrong)
  const uint32_t v = 0x3C003C00u + lane;
#pragma unroll
  for (int piece = 0; piece < prec_pieces(PREC); ++piece) t.p[piece] = u32x4{v, v, v, v};
  asm volatile("" :: "v"(w));
#else
  // uniform base + unsigned 32-bit lane offset: the loads take their base from scalar registers (no 64-bit address per
  // tap).  The offset is opaque to the optimiser, which would otherwise fold it into a per-lane base outside the job loop.
  unsigned off = (unsigned)lane * 16u;
  asm volatile("" : "+v"(off));
  typedef const __attribute__((address_space(1))) u32x4* gptr;   // global (not flat) loads: vmcnt only
  unsigned long long b = reinterpret_cast<unsigned long long>(w);
  asm volatile("" : "+s"(b));                              // the tap's base stays a scalar: base + lane offset + immediate
  t.p[0] = *reinterpret_cast<gptr>(b + off);
  if constexpr (PREC == PREC_F32) {
    t.p[1] = *reinterpret_cast<gptr>(b + off + 1024);
    t.p[2] = *reinterpret_cast<gptr>(b + off + 2048);
  }
#endif
}
template <int PREC>
__device__ __forceinline__ void load_b(FragST<PREC>& f, const float* __restrict__ w, int lane) {   // a whole K group
#pragma unroll
  for (int i = 0; i < W_RING; ++i) load_tap(f.rb[i], w + i * tap_dwords(PREC), lane);
}
template <int PREC>
__device__ __forceinline__ void zero_b(FragST<PREC>& f) {
#pragma unroll
  for (int t = 0; t < W_RING; ++t)
#pragma unroll
    for (int piece = 0; piece < prec_pieces(PREC); ++piece) f.rb[t].p[piece] = u32x4{0u, 0u, 0u, 0u};
}

// the second K group's operands of every cell whose refill_step is STEP (slot address a1)
template <int OMASK, int STEP, int PREC>
__device__ __forceinline__ void refill(PiecesT<PREC> (&x)[CELLS], const unsigned char* __restrict__ src, int a1) {
  if constexpr (refill_step<OMASK, 0>() == STEP) load_cell<OMASK, 0>(x, src, a1);
  if constexpr (refill_step<OMASK, 1>() == STEP) load_cell<OMASK, 1>(x, src, a1);
  if constexpr (refill_step<OMASK, 2>() == STEP) load_cell<OMASK, 2>(x, src, a1);
  if constexpr (refill_step<OMASK, 3>() == STEP) load_cell<OMASK, 3>(x, src, a1);
  if constexpr (refill_step<OMASK, 4>() == STEP) load_cell<OMASK, 4>(x, src, a1);
  if constexpr (refill_step<OMASK, 5>() == STEP) load_cell<OMASK, 5>(x, src, a1);
  if constexpr (refill_step<OMASK, 6>() == STEP) load_cell<OMASK, 6>(x, src, a1);
  if constexpr (refill_step<OMASK, 7>() == STEP) load_cell<OMASK, 7>(x, src, a1);
  if constexpr (refill_step<OMASK, 8>() == STEP) load_cell<OMASK, 8>(x, src, a1);
}
// One K group (32 channels), tap-major.  The weight ring holds three taps: tap t's operands sit in slot t % 3 and, once
// its MFMAs are issued, the slot is refilled with tap t + 3 -- of this K group (`wc`) or, for the last three taps, with
// taps 0-2 of the NEXT K group (`wn`; when nothing follows, any readable weights: the loads are unconditional) -- so the
// weight stream runs three taps ahead, also across jobs and stage barriers.  PART 1 / 2: the first / second K group of a
// two-group job -- the activation operands of the second group are read in place (LDS slot address a1) at their
// refill_step, some after a tap of the first group, the others before a tap of the second; PART 0: a one-group job.
// `e`: the epilogue scheduler of the job's LAST K group (PART 0 / 2; NoEpi for PART 1).
template <int OMASK, int PART, typename E, int PREC>
__device__ __forceinline__ void kgroup(f32x4 (&acc)[CELLS], Operands<OMASK, PREC>& xs, FragST<PREC>& f,
                                       const unsigned char* __restrict__ src, int a1,
                                       const float* __restrict__ wc, const float* __restrict__ wn, int lane, E& e) {
  constexpr bool A = PART == 1, B = PART == 2;
  constexpr int TAP_DWORDS = tap_dwords(PREC);        // (of this mode's stream)
  PiecesT<PREC> (&x)[CELLS] = xs.x;
  if constexpr (B) refill<OMASK, 9>(x, src, a1);
  tap_mfma<OMASK, 0, PART>(acc, xs, f.rb[0], e); load_tap(f.rb[0], wc + 3 * TAP_DWORDS, lane);
  if constexpr (A) refill<OMASK, 0>(x, src, a1);
  if constexpr (B) refill<OMASK, 10>(x, src, a1);
  tap_mfma<OMASK, 1, PART>(acc, xs, f.rb[1], e); load_tap(f.rb[1], wc + 4 * TAP_DWORDS, lane);
  if constexpr (A) refill<OMASK, 1>(x, src, a1);
  if constexpr (B) refill<OMASK, 11>(x, src, a1);
  tap_mfma<OMASK, 2, PART>(acc, xs, f.rb[2], e); load_tap(f.rb[2], wc + 5 * TAP_DWORDS, lane);
  if constexpr (A) refill<OMASK, 2>(x, src, a1);
  if constexpr (B) refill<OMASK, 12>(x, src, a1);
  tap_mfma<OMASK, 3, PART>(acc, xs, f.rb[0], e); load_tap(f.rb[0], wc + 6 * TAP_DWORDS, lane);
  if constexpr (A) refill<OMASK, 3>(x, src, a1);
  if constexpr (B) refill<OMASK, 13>(x, src, a1);
  tap_mfma<OMASK, 4, PART>(acc, xs, f.rb[1], e); load_tap(f.rb[1], wc + 7 * TAP_DWORDS, lane);
  if constexpr (A) refill<OMASK, 4>(x, src, a1);
  if constexpr (B) refill<OMASK, 14>(x, src, a1);
  tap_mfma<OMASK, 5, PART>(acc, xs, f.rb[2], e); load_tap(f.rb[2], wc + 8 * TAP_DWORDS, lane);
  if constexpr (A) refill<OMASK, 5>(x, src, a1);
  if constexpr (B) refill<OMASK, 15>(x, src, a1);
  tap_mfma<OMASK, 6, PART>(acc, xs, f.rb[0], e); load_tap(f.rb[0], wn + 0 * TAP_DWORDS, lane);
  if constexpr (A) refill<OMASK, 6>(x, src, a1);
  if constexpr (B) refill<OMASK, 16>(x, src, a1);
  tap_mfma<OMASK, 7, PART>(acc, xs, f.rb[1], e); load_tap(f.rb[1], wn + 1 * TAP_DWORDS, lane);
  if constexpr (A) refill<OMASK, 7>(x, src, a1);
  if constexpr (B) refill<OMASK, 17>(x, src, a1);
  tap_mfma<OMASK, 8, PART>(acc, xs, f.rb[2], e); load_tap(f.rb[2], wn + 2 * TAP_DWORDS, lane);
  if constexpr (A) refill<OMASK, 8>(x, src, a1);
}
// All K groups of one job as straight-line code (KG = 1 or 2: layers are at most 64 channels wide;
// a loop would carry the operand registers around its back edge through copies).  On entry the
// ring holds the first three taps of the job's first K group; on exit those of the next job that reads
// weights (`w_after`; the stream's start when there is none).  The K groups start at slot `sslot` of the source rows
// (NET_SSLOT_SPLIT: one K group from two areas, load_cells_split).
template <int OMASK, int KG, typename E, int PREC>
__device__ __forceinline__ void job_kloop(f32x4 (&acc)[CELLS], FragST<PREC>& f, const unsigned char* __restrict__ src,
                                          const unsigned char* __restrict__ strip, int sslot,
                                          const float* __restrict__ w, const float* __restrict__ w_after, int lane, E& e) {
  const int pos = lane & 15, quad = lane >> 4;
  Operands<OMASK, PREC> xs;
  if (KG == 1 && OMASK != 0x1FF && sslot == NET_SSLOT_SPLIT) load_cells_split<OMASK>(xs.x, src, strip, pos, quad);   // (no whole-tile job reads the strip)
  else load_cells<OMASK>(xs.x, src, slot_addr(0, pos, sslot + quad));
  if constexpr (Operands<OMASK, PREC>::NP == 2) {          // piece 2 of the first pairs
    xs.src = src;
    xs.cur = slot_addr(0, pos, sslot + quad);
    xs.nxt = slot_addr(0, pos, sslot + 4 + quad);
    xs.template fetch_third<0, KG == 2 ? 1 : 0>();
    xs.template fetch_third<1, KG == 2 ? 1 : 0>();
    static_assert(LATE_AHEAD == 2, "the pairs fetched before the K loop");
  }
  if constexpr (KG == 2) {
    const int a1 = slot_addr(0, pos, sslot + 4 + quad);
    NoEpi none;
    kgroup<OMASK, 1>(acc, xs, f, src, a1, w, w + kg_dwords(PREC), lane, none);
    if constexpr (Operands<OMASK, PREC>::NP == 2) xs.cur = a1;
    kgroup<OMASK, 2>(acc, xs, f, src, a1, w + kg_dwords(PREC), w_after, lane, e);
  } else {
    kgroup<OMASK, 0>(acc, xs, f, src, 0, w, w_after, lane, e);
  }
}

// tanh for the value head: 1 - 2 / (exp(2x) + 1) on the hardware exp; absolute error < 3e-7
// (the parity tolerance on values is 1e-5), exact limits at +-inf
__device__ __forceinline__ float tanh_fast(float x) { return 1.0f - 2.0f / (__expf(2.0f * x) + 1.0f); }

template <int OMASK, int TAP, int I>
__device__ __forceinline__ void mfma_extra_pair(f32x4 (&acc)[CELLS], const float (&ax)[CELLS], const float (&bx)[9]) {
  if constexpr (pair_used<OMASK, I, TAP>()) {
    constexpr int o = TapMap<I, TAP>::o;
    acc[o] = __builtin_amdgcn_mfma_f32_16x16x4f32(bx[TAP], ax[I], acc[o], 0, 0, 0);
  }
}
template <int OMASK, int TAP>
__device__ __forceinline__ void mfma_extra_tap(f32x4 (&acc)[CELLS], const float (&ax)[CELLS], const float (&bx)[9]) {
  mfma_extra_pair<OMASK, TAP, 0>(acc, ax, bx); mfma_extra_pair<OMASK, TAP, 1>(acc, ax, bx);
  mfma_extra_pair<OMASK, TAP, 2>(acc, ax, bx); mfma_extra_pair<OMASK, TAP, 3>(acc, ax, bx);
  mfma_extra_pair<OMASK, TAP, 4>(acc, ax, bx); mfma_extra_pair<OMASK, TAP, 5>(acc, ax, bx);
  mfma_extra_pair<OMASK, TAP, 6>(acc, ax, bx); mfma_extra_pair<OMASK, TAP, 7>(acc, ax, bx);
  mfma_extra_pair<OMASK, TAP, 8>(acc, ax, bx);
}
// the (<= 4) raw input planes as one extra K step in plain float32 (projection / recall conv):
// lane l supplies W[cout = l & 15][plane = l >> 4] and X[plane = l >> 4][pos = l & 15]
template <int OMASK>
__device__ __forceinline__ void extra_planes(f32x4 (&acc)[CELLS], const float* __restrict__ wx,
                                             const float* __restrict__ inp, int lane) {
  float ax[CELLS], bx[9];
  // (explicit address spaces: a FLAT load in flight makes every later wait in the job a full vmcnt(0) / lgkmcnt(0))
  const __attribute__((address_space(1))) float* wxg = (const __attribute__((address_space(1))) float*)wx;
  const __attribute__((address_space(3))) float* inl = (const __attribute__((address_space(3))) float*)inp;
#pragma unroll
  for (int t = 0; t < 9; ++t) bx[t] = wxg[t * 64 + lane];
#pragma unroll
  for (int i = 0; i < CELLS; ++i) ax[i] = inl[(i * POS + (lane & 15)) * 4 + (lane >> 4)];
  mfma_extra_tap<OMASK, 0>(acc, ax, bx); mfma_extra_tap<OMASK, 1>(acc, ax, bx); mfma_extra_tap<OMASK, 2>(acc, ax, bx);
  mfma_extra_tap<OMASK, 3>(acc, ax, bx); mfma_extra_tap<OMASK, 4>(acc, ax, bx); mfma_extra_tap<OMASK, 5>(acc, ax, bx);
  mfma_extra_tap<OMASK, 6>(acc, ax, bx); mfma_extra_tap<OMASK, 7>(acc, ax, bx); mfma_extra_tap<OMASK, 8>(acc, ax, bx);
}

// ---- epilogues: lane holds C[cout = 16 nt + 4 quad + r][pos = lane & 15] for the job's cells ------
// ACT: 0 none, 1 relu, 2 tanh, 3 elu.  The four channels of a lane are half a 16-byte slot: one
// ds_write_b64 per piece (and one ds_read_b64 per piece for the residual, which the three pieces
// reproduce exactly).  Output cell o lives o * 2048 bytes after cell 0.
// STRIP: dst is the strip (its only tile; nt is ignored).
// first MFMA slot of the last K group (slot g follows its g-th MFMA) for the steps of the qi-th early cell, `ns` steps a
// cell: not before the first MFMA of the tap after the cell's final one, and after the cell queued before it
constexpr int early_begin(int omask, int ns, int qi) {
  int b = 0, end = 0;
  for (int q = 0; q <= qi; ++q) {
    const int start = 6 * pairs_before(omask, net_final_tap(early_cell(omask, q)) + 1, 0);
    b = start > end ? start : end;
    end = b + ns;
  }
  return b;
}
// the whole queue of a group: its early cells and their first slots, worked out once per ProgEpi instantiation
constexpr int EPI_QUEUE = 5;          // cells final before tap 8: 2, 5, 6, 7, 8
struct EpiQueue {
  int n, cell[EPI_QUEUE], begin[EPI_QUEUE];
};
constexpr EpiQueue epi_queue(int omask, int ns) {
  EpiQueue q{};
  q.n = early_cells(omask);
  for (int i = 0; i < EPI_QUEUE; ++i) {
    q.cell[i] = i < q.n ? early_cell(omask, i) : 0;
    q.begin[i] = i < q.n ? early_begin(omask, ns, i) : 0;
  }
  return q;
}
// One cell's epilogue is a fixed sequence of steps of a few VALU instructions each, so that the K loop can issue it step
// by step between its MFMAs (ProgEpi) and the end-of-job form runs the very same steps back to back (epilogue_cell):
//   residual (RES: 8 steps, per channel the three pieces' conversion, then the sum; else one empty step, which keeps a
//   cell's first read of its accumulator an MFMA away from the MFMA that wrote it) | activation (tanh, elu: one step per
//   channel; else one) | split and store (7: piece 0, remainders of channels 0-1, of 2-3, piece 1, again, piece 2)
template <int ACT, bool RES>
constexpr int epi_steps() { return (RES ? 8 : 1) + (ACT >= 2 ? 4 : 1) + 7; }
struct EpiRegs {
  f32x4 v;          // the four channels: accumulator (+ residual), activated
  u32x2 q[3];       // the residual's three pieces
  float c[3];
  float r[4];       // remainders of the split
};
template <int ACT>
__device__ __forceinline__ float epi_act(float x) {
  if constexpr (ACT == 1) x = fmaxf(x, 0.0f);
  if constexpr (ACT == 2) x = tanh_fast(x);
  if constexpr (ACT == 3) x = x > 0.0f ? x : expm1f(x);      // nn.ELU(), alpha = 1
  return x;
}
__device__ __forceinline__ float epi_rem(float x) { return x - bf16_trunc(x); }
// this lane's byte offset inside cell 0 of one piece: half a 16-byte slot (four channels)
template <bool STRIP>
__device__ __forceinline__ int epi_off(int lane, int nt) {
  const int pos = lane & 15, quad = lane >> 4;
  return (STRIP ? strip_addr(0, pos, quad >> 1) : slot_addr(0, pos, nt * 2 + (quad >> 1))) + (quad & 1) * 8;
}
template <int O>
__device__ __forceinline__ void epi_read_res(u32x2 (&q)[3], const unsigned char* res, int off) {
#pragma unroll
  for (int piece = 0; piece < 3; ++piece)
    q[piece] = *reinterpret_cast<const u32x2*>(res + piece * PIECE_BYTES + O * (POS * 128) + off);
}
// step K of cell O: `a` is its accumulator
template <int ACT, bool RES, bool STRIP, int O, int K>
__device__ __forceinline__ void epi_step(EpiRegs& s, const f32x4& a, unsigned char* __restrict__ dst, int off) {
  constexpr int PB = STRIP ? STRIP_PIECE_BYTES : PIECE_BYTES, CB = STRIP ? POS * 32 : POS * 128;
  constexpr int NR = RES ? 8 : 1, NA = ACT >= 2 ? 4 : 1;
  static_assert(K >= 0 && K < NR + NA + 7, "step of the sequence");
  if constexpr (K < NR) {
    if constexpr (RES) {
      constexpr int r = K >> 1;                  // channel: word r / 2 of each piece, its low (even r) or high half
      if constexpr ((K & 1) == 0) {
#pragma unroll
        for (int piece = 0; piece < 3; ++piece) s.c[piece] = (r & 1) ? bf16_hi(s.q[piece][r >> 1]) : bf16_lo(s.q[piece][r >> 1]);
      } else {
        s.v[r] = a[r] + ((s.c[0] + s.c[1]) + s.c[2]);
      }
    }
  } else if constexpr (K < NR + NA) {
    if constexpr (NA == 4) {
      constexpr int r = K - NR;
      s.v[r] = epi_act<ACT>(RES ? s.v[r] : a[r]);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) s.v[r] = epi_act<ACT>(RES ? s.v[r] : a[r]);
    }
  } else {
    constexpr int P = K - NR - NA;
    unsigned char* const d = dst + O * CB + off;
    if constexpr (P == 0) *reinterpret_cast<u32x2*>(d + 0 * PB) = u32x2{pack_hi16(s.v[0], s.v[1]), pack_hi16(s.v[2], s.v[3])};
    if constexpr (P == 1) { s.r[0] = epi_rem(s.v[0]); s.r[1] = epi_rem(s.v[1]); }
    if constexpr (P == 2) { s.r[2] = epi_rem(s.v[2]); s.r[3] = epi_rem(s.v[3]); }
    if constexpr (P == 3) *reinterpret_cast<u32x2*>(d + 1 * PB) = u32x2{pack_hi16(s.r[0], s.r[1]), pack_hi16(s.r[2], s.r[3])};
    if constexpr (P == 4) { s.r[0] = epi_rem(s.r[0]); s.r[1] = epi_rem(s.r[1]); }
    if constexpr (P == 5) { s.r[2] = epi_rem(s.r[2]); s.r[3] = epi_rem(s.r[3]); }
    if constexpr (P == 6) *reinterpret_cast<u32x2*>(d + 2 * PB) = u32x2{pack_hi16(s.r[0], s.r[1]), pack_hi16(s.r[2], s.r[3])};
  }
}
// steps K0 .. the last of cell O
template <int ACT, bool RES, bool STRIP, int O, int K0>
__device__ __forceinline__ void epi_steps_from(EpiRegs& s, const f32x4& a, unsigned char* __restrict__ dst, int off) {
  if constexpr (K0 < epi_steps<ACT, RES>()) {
    epi_step<ACT, RES, STRIP, O, K0>(s, a, dst, off);
    epi_steps_from<ACT, RES, STRIP, O, K0 + 1>(s, a, dst, off);
  }
}
// the whole epilogue of one cell; `q`: its residual pieces, already read (RES)
template <int O, int ACT, bool RES, bool STRIP>
__device__ __forceinline__ void epilogue_cell(const f32x4& a, const u32x2 (&q)[3], unsigned char* __restrict__ dst, int off) {
  EpiRegs s;
  if constexpr (RES) { s.q[0] = q[0]; s.q[1] = q[1]; s.q[2] = q[2]; }
  epi_steps_from<ACT, RES, STRIP, O, 0>(s, a, dst, off);
}
// the cells of CMASK at the end of the job: all residual reads in flight at once, before any write
template <int CMASK, int ACT, bool RES, bool STRIP, int O = 0>
__device__ __forceinline__ void epilogue_cells(const f32x4 (&acc)[CELLS], const u32x2 (&q)[CELLS][3],
                                               unsigned char* __restrict__ dst, int off) {
  if constexpr (O < CELLS) {
    if constexpr ((CMASK >> O) & 1) epilogue_cell<O, ACT, RES, STRIP>(acc[O], q[O], dst, off);
    epilogue_cells<CMASK, ACT, RES, STRIP, O + 1>(acc, q, dst, off);
  }
}
template <int CMASK, int O = 0>
__device__ __forceinline__ void epi_read_cells(u32x2 (&q)[CELLS][3], const unsigned char* res, int off) {
  if constexpr (O < CELLS) {
    if constexpr ((CMASK >> O) & 1) epi_read_res<O>(q[O], res, off);
    epi_read_cells<CMASK, O + 1>(q, res, off);
  }
}
// Plain-bf16 mode, one cell: the residual is the STORED bf16 value, widened; the float32 mode's activation; one rounding
// to nearest even and one 8-byte store into piece plane 0.
template <int O, int ACT, bool RES, bool STRIP>
__device__ __forceinline__ void epilogue_cell_bf16(const f32x4& a, const u32x2& q, unsigned char* __restrict__ dst, int off) {
  constexpr int CB = STRIP ? POS * 32 : POS * 128;
  f32x4 v = a;
  if constexpr (RES) {
    v[0] = a[0] + bf16_lo(q[0]); v[1] = a[1] + bf16_hi(q[0]);
    v[2] = a[2] + bf16_lo(q[1]); v[3] = a[3] + bf16_hi(q[1]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = epi_act<ACT>(v[r]);
  *reinterpret_cast<u32x2*>(dst + O * CB + off) = u32x2{pack_rne16(v[0], v[1]), pack_rne16(v[2], v[3])};
}
template <int CMASK, int ACT, bool RES, bool STRIP, int O = 0>
__device__ __forceinline__ void epilogue_cells_bf16(const f32x4 (&acc)[CELLS], const u32x2 (&q)[CELLS],
                                                    unsigned char* __restrict__ dst, int off) {
  if constexpr (O < CELLS) {
    if constexpr ((CMASK >> O) & 1) epilogue_cell_bf16<O, ACT, RES, STRIP>(acc[O], q[O], dst, off);
    epilogue_cells_bf16<CMASK, ACT, RES, STRIP, O + 1>(acc, q, dst, off);
  }
}
template <int OMASK, int ACT, bool RES, bool STRIP = false, int PREC = PREC_F32>
__device__ __forceinline__ void epilogue_lds(const f32x4 (&acc)[CELLS], unsigned char* __restrict__ dst,
                                             const unsigned char* res, int lane, int nt) {
  const int off = epi_off<STRIP>(lane, nt);
  if constexpr (PREC == PREC_BF16) {      // all residual reads in flight at once, before any write, as below
    u32x2 q1[CELLS];
    if constexpr (RES) {
#pragma unroll
      for (int o = 0; o < CELLS; ++o)
        if ((OMASK >> o) & 1) q1[o] = *reinterpret_cast<const u32x2*>(res + o * (POS * 128) + off);
    }
    epilogue_cells_bf16<OMASK, ACT, RES, STRIP>(acc, q1, dst, off);
    return;
  }
#ifdef NZ_ABLATE_EPI   // timing-only build: one store per job instead of the epilogue (outputs are wrong)
  {
    float t = 0.f;
#pragma unroll
    for (int o = 0; o < CELLS; ++o) if ((OMASK >> o) & 1) t += acc[o][0] + acc[o][1] + acc[o][2] + acc[o][3];
    *reinterpret_cast<float*>(dst + off) = t;
    return;
  }
#endif
  u32x2 q[CELLS][3];
  if constexpr (RES) epi_read_cells<OMASK>(q, res, off);
  epilogue_cells<OMASK, ACT, RES, STRIP>(acc, q, dst, off);
}

// Progressive epilogue (NetJob flag NET_JOB_PROGRESSIVE; destination an activation buffer).  The job's early cells are
// queued in the order they become final; cell qi's steps take the MFMA slots of the last K group from `begin(qi)` on, one
// step per slot: not before the first MFMA of the tap after its final one, and after the cell queued before it.  Its
// residual pieces are read READ_AHEAD slots earlier (the registers are free: the previous cell is past its residual
// steps), so the wait in front of its first use is a counted one on loads a whole chain old.  Every slot with work is
// fenced: the steps stay between the two MFMAs they were placed between, and each six-MFMA chain stays one chain.  What
// the K loop has no slots left for, and the cells final at tap 8, run at the end of the job (`finish`).  No work moves
// between waves, nothing is read or computed twice: per cell the same steps on the same values as epilogue_cell.
template <int OMASK, int ACT, bool RES>
struct ProgEpi {
  static constexpr int NS = epi_steps<ACT, RES>(), NQ = early_cells(OMASK), SLOTS = 6 * pairs_before(OMASK, 9, 0);
  static constexpr int READ_AHEAD = 6;
  static constexpr int LATE = OMASK & 0x01B;          // cells 0, 1, 3, 4: final at tap 8
  static_assert(NQ >= 1 && NQ <= EPI_QUEUE, "groups with early cells");
  static constexpr EpiQueue Q = epi_queue(OMASK, NS);
  static constexpr int FIRST = RES ? Q.begin[0] - READ_AHEAD : Q.begin[0];     // the first slot with work: `off` is derived there
  static_assert(FIRST >= 0 && FIRST < SLOTS && (!RES || READ_AHEAD <= NS - 8), "reads land inside the K group, behind the residual steps");
  static constexpr int cell(int qi) { return Q.cell[qi]; }
  static constexpr int begin(int qi) { return Q.begin[qi]; }
  static constexpr int read_slot(int qi) { return begin(qi) - READ_AHEAD; }

  EpiRegs s;
  unsigned char* dst;
  const unsigned char* res;
  int lane, nt, off;

  template <int QI, int G>
  __device__ __forceinline__ void slot_of(const f32x4 (&acc)[CELLS]) {
    if constexpr (QI < NQ) {
      if constexpr (RES && G == read_slot(QI)) epi_read_res<cell(QI)>(s.q, res, off);
      if constexpr (G >= begin(QI) && G < begin(QI) + NS) epi_step<ACT, RES, false, cell(QI), G - begin(QI)>(s, acc[cell(QI)], dst, off);
    }
  }
  template <int QI, int G>
  static constexpr bool busy() {
    if constexpr (QI < NQ) return (RES && G == read_slot(QI)) || (G >= begin(QI) && G < begin(QI) + NS);
    return false;
  }
  template <int G>
  __device__ __forceinline__ void slot(const f32x4 (&acc)[CELLS]) {
    if constexpr (busy<0, G>() || busy<1, G>() || busy<2, G>() || busy<3, G>() || busy<4, G>()) {
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (G == FIRST) off = epi_off<false>(lane, nt);
      slot_of<0, G>(acc); slot_of<1, G>(acc); slot_of<2, G>(acc); slot_of<3, G>(acc); slot_of<4, G>(acc);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // after the K loop: what is left of the early cells, in queue order, then the cells final at tap 8
  template <int QI>
  __device__ __forceinline__ void finish_early(const f32x4 (&acc)[CELLS]) {
    if constexpr (QI < NQ) {
      if constexpr (RES && read_slot(QI) >= SLOTS) epi_read_res<cell(QI)>(s.q, res, off);
      constexpr int done = SLOTS - begin(QI);
      epi_steps_from<ACT, RES, false, cell(QI), (done > 0 ? done : 0)>(s, acc[cell(QI)], dst, off);
      finish_early<QI + 1>(acc);
    }
  }
  __device__ __forceinline__ void finish(const f32x4 (&acc)[CELLS]) {
    u32x2 q[CELLS][3];
    if constexpr (RES) epi_read_cells<LATE>(q, res, off);
    finish_early<0>(acc);
    epilogue_cells<LATE, ACT, RES, false>(acc, q, dst, off);
  }
};

// (whole-tile jobs, group 0, go to an activation buffer only: engine.hip solo_list)
template <int OMASK, int PREC = PREC_F32>
__device__ __forceinline__ void epilogue(const f32x4 (&acc)[CELLS], const NetJob& job, unsigned char* __restrict__ lds,
                                         unsigned char* __restrict__ strip, int lane, int policy_channels, int n_valid,
                                         float* logits, float* vcells) {
  constexpr bool BUFFER_ONLY = OMASK == 0x1FF;
  if (!BUFFER_ONLY && job.dst == NET_DST_STRIP) {             // ReLU only: the host compiles nothing else into the strip
    epilogue_lds<OMASK, 1, false, true, PREC>(acc, strip, nullptr, lane, 0);
  } else if (BUFFER_ONLY || job.dst < NET_BUFFERS) {
    unsigned char* dst = lds + job.dst * ACT_BYTES;
    if (job.res >= 0) {
      epilogue_lds<OMASK, 1, true, false, PREC>(acc, dst, lds + job.res * ACT_BYTES, lane, job.dtile);
    } else if (job.act == 1) {
      epilogue_lds<OMASK, 1, false, false, PREC>(acc, dst, nullptr, lane, job.dtile);
    } else if (job.act == 2) {
      epilogue_lds<OMASK, 2, false, false, PREC>(acc, dst, nullptr, lane, job.dtile);
    } else if (job.act == 3) {
      epilogue_lds<OMASK, 3, false, false, PREC>(acc, dst, nullptr, lane, job.dtile);
    } else {
      epilogue_lds<OMASK, 0, false, false, PREC>(acc, dst, nullptr, lane, job.dtile);
    }
  } else if (job.dst == NET_DST_POLICY) {     // policy logits [pos][P][9]
    // (addresses re-derived from an opaque copy of the lane id: hoisted out of the job loop they would sit in
    // registers -- in the persistent kernel: in scratch memory -- for the whole network)
    int l2 = lane;
    asm volatile("" : "+v"(l2));
    const int pos = l2 & 15, quad = l2 >> 4;
    if (pos < n_valid) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int cout = job.nt * 16 + quad * 4 + r;
        if (cout < policy_channels) {
#pragma unroll
          for (int o = 0; o < CELLS; ++o)
            if ((OMASK >> o) & 1) logits[((size_t)pos * policy_channels + cout) * CELLS + o] = acc[o][r];
        }
      }
    }
  } else {                                     // value: channel 0 of every cell; net_tile takes the mean when all are in
    int l2 = lane;                             // as for the policy: no address hoisted out of the job loop
    asm volatile("" : "+v"(l2));
    const int pos = l2 & 15, quad = l2 >> 4;
    if (job.nt == 0 && quad == 0) {
#pragma unroll
      for (int o = 0; o < CELLS; ++o)
        if ((OMASK >> o) & 1) vcells[o * POS + pos] = acc[o][0];
    }
  }
}

// one job: K loop, input-plane step, epilogue
template <int OMASK, typename Stamp, typename Fetch, int PREC>
__device__ __forceinline__ void run_job_plain(const NetJob& job, FragST<PREC>& f, const float* __restrict__ W,
                                              const float* w_after, unsigned char* __restrict__ lds,
                                              unsigned char* __restrict__ strip,
                                              const float* __restrict__ inp, int lane, int policy_channels, int n_valid,
                                              float* logits, float* value, Stamp&& stamp, Fetch&& fetch_next) {
  // per-lane LDS addresses are derived inside the job from an opaque copy of the lane id: hoisted out of the job loop
  // they are spilled and reloaded in the middle of the K loop, behind a wait for the whole weight stream
  asm volatile("" : "+v"(lane));
  f32x4 acc[CELLS];
#pragma unroll
  for (int o = 0; o < CELLS; ++o) acc[o] = f32x4{0.f, 0.f, 0.f, 0.f};
  NoEpi none;
  if (job.kgroups == 2) job_kloop<OMASK, 2>(acc, f, lds + job.src * ACT_BYTES, strip, job.sslot, W + job.w_off, w_after, lane, none);
  else if (job.kgroups == 1) job_kloop<OMASK, 1>(acc, f, lds + job.src * ACT_BYTES, strip, job.sslot, W + job.w_off, w_after, lane, none);
  stamp(0);
  if (job.extra) extra_planes<OMASK>(acc, W + job.wx_off, inp, lane);
  stamp(1);
  fetch_next();          // the next job's descriptor: in flight under the epilogue, in no register during the K loop
  epilogue<OMASK, PREC>(acc, job, lds, strip, lane, policy_channels, n_valid, logits, value);   // `value`: the per-cell staging area
  stamp(2);
}
// a job flagged NET_JOB_PROGRESSIVE: one or two K groups from a buffer, no input planes, destination a buffer; the
// epilogue kind is fixed before the K loop
template <int OMASK, int ACT, bool RES, typename Stamp, typename Fetch>
__device__ __forceinline__ void run_job_prog(const NetJob& job, FragS& f, const float* __restrict__ W,
                                             const float* w_after, unsigned char* __restrict__ lds,
                                             unsigned char* __restrict__ strip, int lane, Stamp&& stamp, Fetch&& fetch_next) {
  asm volatile("" : "+v"(lane));                // as in run_job_plain
  f32x4 acc[CELLS];
#pragma unroll
  for (int o = 0; o < CELLS; ++o) acc[o] = f32x4{0.f, 0.f, 0.f, 0.f};
  ProgEpi<OMASK, ACT, RES> e;
  e.dst = lds + job.dst * ACT_BYTES;
  e.res = lds + (RES ? job.res : 0) * ACT_BYTES;
  e.lane = lane;
  e.nt = job.dtile;
  if (job.kgroups == 2) job_kloop<OMASK, 2>(acc, f, lds + job.src * ACT_BYTES, strip, job.sslot, W + job.w_off, w_after, lane, e);
  else job_kloop<OMASK, 1>(acc, f, lds + job.src * ACT_BYTES, strip, job.sslot, W + job.w_off, w_after, lane, e);
  stamp(0);
  stamp(1);
  fetch_next();
  e.finish(acc);
  stamp(2);
}
template <int OMASK, typename Stamp, typename Fetch, int PREC>
__device__ __forceinline__ void run_job(const NetJob& job, FragST<PREC>& f, const float* __restrict__ W,
                                        const float* w_after, unsigned char* __restrict__ lds,
                                        unsigned char* __restrict__ strip,
                                        const float* __restrict__ inp, int lane, int policy_channels, int n_valid,
                                        float* logits, float* value, Stamp&& stamp, Fetch&& fetch_next) {
#ifndef NZ_ABLATE_EPI
  if constexpr (PREC == PREC_F32 && net_og_progressive(OMASK)) {     // (plain-bf16: end-of-job epilogues, the same values)
    if (job.flags & NET_JOB_PROGRESSIVE) {      // (engine.hip add_stage: ReLU with or without residual, or tanh)
      if (job.res >= 0) run_job_prog<OMASK, 1, true>(job, f, W, w_after, lds, strip, lane, stamp, fetch_next);
      else if (job.act == 2) run_job_prog<OMASK, 2, false>(job, f, W, w_after, lds, strip, lane, stamp, fetch_next);
      else run_job_prog<OMASK, 1, false>(job, f, W, w_after, lds, strip, lane, stamp, fetch_next);
      return;
    }
  }
#endif
  run_job_plain<OMASK>(job, f, W, w_after, lds, strip, inp, lane, policy_channels, n_valid, logits, value, stamp, fetch_next);
}

// value = tanh(mean over (C=1,H,W)) (blocks.py:82-84); the last stage's jobs left channel 0 of each cell in `vcells`
// (the program's last stage ends with a barrier).  Cells are added in index order, whichever wave produced them.
__device__ __forceinline__ void net_value_mean(const float* lds_f, int tid, int n_valid, float* value) {
  const float* const vcells = lds_f + NET_BUFFERS * ACT_FLOATS + INP_FLOATS;
  if (tid < POS && tid < n_valid) {
    float sum = 0.0f;
#pragma unroll
    for (int o = 0; o < CELLS; ++o) sum += vcells[o * POS + tid];
    value[tid] = tanh_fast(sum / 9.0f);
  }
}

// Run the compiled network on the 16 positions whose input planes are in `inp`
// ([cell][pos][4 planes]); `lds_f` holds the activation buffers (NET_BUFFERS * ACT_FLOATS floats,
// no NaN bit patterns: the callers zero it once), then `inp`'s INP_FLOATS, then VAL_FLOATS of staging, then the
// strip's STRIP_FLOATS (zeroed once as well).  Every thread of the 256-thread workgroup must
// call it; it ends with a workgroup barrier.
// Outputs: logits [pos][policy_channels][9] and value [pos] for pos < n_valid
// (any address space).
// STAMPS (diagnostic build only): wave 0 adds up the shader-clock ticks it spends in the K
// loops, the input-plane step, the epilogues and at the stage barriers into stamps[0..3].
// `steal` (uniform per wave; the persistent kernel only): wave w ^ 4, the other wave of this SIMD, sits the pass out
// (selfplay.hip burst_under_pass) and this wave runs its jobs too: it walks its solo list (NetProgram::solo_jobs) instead
// of its own -- stage by stage its own jobs, then the other list's, then the barrier, the two halves of a tile as one
// whole-tile job.  The jobs of a stage are independent of each other, and the progressive-epilogue hazard rule holds for
// the stage as a whole, so which wave runs a job changes nothing it computes.  The job loop is the same for both lists.
// SOLO: the caller may steal, so the whole-tile job is compiled in (the stand-alone network kernel does without it).
// PREC: the arithmetic mode; `W` and the program's weight offsets are that mode's stream.  PREC_BF16 has no stealing pass.
// `after_stage(n)` (the dump kernel only; every thread, after the n-th stage's barrier): copies out what the stage left.
struct NoStageHook {
  __device__ __forceinline__ void operator()(int) const {}
};
template <bool STAMPS = false, bool SOLO = false, int PREC = PREC_F32, typename StageHook = NoStageHook>
__device__ __forceinline__ void net_tile(const NetProgram* __restrict__ prog, const float* __restrict__ W,
                                         float* __restrict__ lds_f, const float* __restrict__ inp,
                                         int policy_channels, int n_valid, float* logits, float* value,
                                         unsigned long long* stamps = nullptr, int steal = 0,
                                         StageHook after_stage = StageHook()) {
  static_assert(PREC == PREC_F32 || !SOLO, "the stolen pass is float32 only");
  unsigned char* __restrict__ lds = reinterpret_cast<unsigned char*>(lds_f);
  float* const vcells = lds_f + NET_BUFFERS * ACT_FLOATS + INP_FLOATS;
  unsigned char* const strip = reinterpret_cast<unsigned char*>(vcells + VAL_FLOATS);
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));                     // per-lane addresses are derived here, not hoisted out of the caller's loop
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const NetJob* __restrict__ jobs = steal ? prog->solo_jobs[wave] : prog->jobs[wave];
  // (uniform by construction; said explicitly for callers that pass `prog` as a generic pointer)
  const int n_jobs = __builtin_amdgcn_readfirstlane(steal ? prog->solo_n_jobs[wave] : prog->n_jobs[wave]);
  const int first_w = __builtin_amdgcn_readfirstlane(steal ? prog->solo_first_w[wave] : prog->first_w_off[wave]);

  FragST<PREC> f;
  zero_b(f);
  if (first_w >= 0) load_b(f, W + first_w, lane);
  int stages_done = 0;

  unsigned long long tk[4] = {0, 0, 0, 0}, ts = 0;
#ifdef NZ_STAGE_STAMPS
  unsigned long long pk[3] = {0, 0, 0}, st_rec[24][3];
  int n_st = 0;
#endif
  auto stamp = [&](int slot) {
    if constexpr (STAMPS) {
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      tk[slot] += now - ts;
      ts = now;
    }
  };
  if constexpr (STAMPS) ts = __builtin_amdgcn_s_memtime();

  // The next job's descriptor is fetched while this job's epilogue runs -- with VECTOR loads (every lane reads the same six
  // words, v_readfirstlane makes them scalars again).  As a scalar load it would share lgkmcnt with the K loop's LDS
  // operand reads and return out of order with them; that variant computes wrong outputs.
  static_assert(sizeof(NetJob) == 24, "six dwords");
  int vzero;
  asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));                  // a zero the compiler must keep in a vector register
  const __attribute__((address_space(1))) uint32_t* jw =
      (const __attribute__((address_space(1))) uint32_t*)reinterpret_cast<const uint32_t*>(jobs) + vzero;   // global, not FLAT
  uint32_t nw[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) nw[i] = jw[i];
  for (int j = 0; j < n_jobs; ++j) {
    NetJob job;
    {
      uint32_t cw[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) cw[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)nw[i]);
      __builtin_memcpy(&job, cw, sizeof(job));
    }
    // Every vector load still in flight here was issued a whole epilogue ago (this job's first three taps): an explicit
    // wait costs nothing and gives the K loop exact counts.  Left to itself the compiler, which cannot count loads across
    // the loop's back edges, makes the first wait inside the job a vmcnt(0) -- behind the taps issued just before it.
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) only
    auto fetch_next = [&]() {
      if (j + 1 < n_jobs) {
#pragma unroll
        for (int i = 0; i < 6; ++i) nw[i] = jw[(j + 1) * 6 + i];
      }
    };
    if (job.og == OG_NONE) fetch_next();
    if (job.og != OG_NONE) {
      const float* w_after = W + (job.next_w_off >= 0 ? job.next_w_off : 0);   // never null: straight-line K loops
      switch (job.og) {
        // (group 0, all nine cells in one job, is never dealt to a wave: layers are at most four tiles wide and eight waves
        // want a unit each -- engine.hip add_stage; a solo list has it where the SIMD's two waves hold a tile's halves)
        case 0: if constexpr (SOLO) run_job<og_mask(0)>(job, f, W, w_after, lds, strip, inp, lane, policy_channels, n_valid, logits, vcells, stamp, fetch_next); break;
        case 1: run_job<og_mask(1)>(job, f, W, w_after, lds, strip, inp, lane, policy_channels, n_valid, logits, vcells, stamp, fetch_next); break;
        case 2: run_job<og_mask(2)>(job, f, W, w_after, lds, strip, inp, lane, policy_channels, n_valid, logits, vcells, stamp, fetch_next); break;
        case 3: run_job<og_mask(3)>(job, f, W, w_after, lds, strip, inp, lane, policy_channels, n_valid, logits, vcells, stamp, fetch_next); break;
        case 4: run_job<og_mask(4)>(job, f, W, w_after, lds, strip, inp, lane, policy_channels, n_valid, logits, vcells, stamp, fetch_next); break;
        case 5: run_job<og_mask(5)>(job, f, W, w_after, lds, strip, inp, lane, policy_channels, n_valid, logits, vcells, stamp, fetch_next); break;
        default: run_job<og_mask(6)>(job, f, W, w_after, lds, strip, inp, lane, policy_channels, n_valid, logits, vcells, stamp, fetch_next); break;
      }
    }
    stamp(2);
    if (job.flags & NET_JOB_STAGE_END) __syncthreads();
    if constexpr (!std::is_same<StageHook, NoStageHook>::value) {
      if (job.flags & NET_JOB_STAGE_END) after_stage(stages_done++);
    }
    stamp(3);
#ifdef NZ_STAGE_STAMPS   // diagnostic build: per-stage ticks of waves 0 and 4 of workgroup 0 (K loops + planes, epilogue, barrier)
    if constexpr (STAMPS) {
      if ((job.flags & NET_JOB_STAGE_END) && blockIdx.x == 0 && (tid == 0 || tid == 256) && n_st < 24) {
        st_rec[n_st][0] = tk[0] + tk[1] - pk[0]; st_rec[n_st][1] = tk[2] - pk[1]; st_rec[n_st][2] = tk[3] - pk[2];
        ++n_st;
        pk[0] = tk[0] + tk[1]; pk[1] = tk[2]; pk[2] = tk[3];
      }
    }
#endif
  }
  net_value_mean(lds_f, tid, n_valid, value);
  __syncthreads();
  if constexpr (STAMPS) {
    if (tid == 0)
      for (int i = 0; i < 4; ++i) stamps[i] = tk[i];
#ifdef NZ_STAGE_STAMPS
    if (blockIdx.x == 0 && (tid == 0 || tid == 256))
      for (int i = 0; i < n_st; ++i)
        printf("wave %d stage %d: k %llu epi %llu bar %llu\n", wave, i, st_rec[i][0], st_rec[i][1], st_rec[i][2]);
#endif
  }
}

}  // namespace nz
