// What the interpreters of a Fused16Program share.  Two kernels run one program: fused16_net_kernel (boardnet.hip), a
// leaf batch on sixteen wavefronts per workgroup, and wave_network (scs_search.hip), one position on the pair of
// wavefronts that owns a game of the persistent SCS self-play kernel.  The two search routes play the same games bit
// for bit only while both do the same float32 operations in the same order, so everything that decides a float is
// written here, once: the split-bf16 arithmetic -- every float32 the exact sum of three bf16 pieces, six of the nine
// piece products on v_mfma_f32_16x16x32_bf16 with float32 accumulation --, the conv taps, the
// layer epilogue's values, the order of the softmax sum, the value's tanh(mean), and the layer program the host
// resolves (every LDS offset and stride) with the way its descriptors reach scalar registers.  Each kernel keeps its
// own schedule, LDS layout, addresses and store predicates.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "bf16_split.hpp"

namespace nz {

// ---- conv taps ------------------------------------------------------------------------------------------------------------
// Square: tap = 3 (dy + 1) + (dx + 1).  Hexagonal (hexagdly's addressing: odd columns sit half a cell lower): 0 N,
// 1 centre, 2 S (same column), 3 NW, 4 SW (column - 1), 5 NE, 6 SE (column + 1); the upper / lower neighbour in an
// adjacent column is row - 1 / row for a cell in an even column, row / row + 1 in an odd one.  `cx`: the cell's column.
template <bool HEX>
__host__ __device__ constexpr int tap_count() { return HEX ? 7 : 9; }
template <bool HEX>
__host__ __device__ constexpr int tap_dy(int tap, int cx) {
  return HEX ? (tap < 3 ? tap - 1 : ((tap - 3) & 1) - 1 + (cx & 1)) : tap / 3 - 1;
}
template <bool HEX>
__host__ __device__ constexpr int tap_dx(int tap) { return HEX ? (tap < 3 ? 0 : (tap < 5 ? -1 : 1)) : tap % 3 - 1; }

constexpr bool square_taps_ok() {          // the nine taps are {-1, 0, 1}^2 in the order 3 (dy + 1) + (dx + 1), in every column
  for (int cx = 0; cx < 2; ++cx)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int tap = 3 * (dy + 1) + (dx + 1);
        if (tap_dy<false>(tap, cx) != dy || tap_dx<false>(tap) != dx) return false;
      }
  return true;
}
constexpr bool hex_taps_distinct(int cx) {   // seven different offsets, the centre at tap 1
  for (int a = 0; a < 7; ++a)
    for (int b = a + 1; b < 7; ++b)
      if (tap_dy<true>(a, cx) == tap_dy<true>(b, cx) && tap_dx<true>(a) == tap_dx<true>(b)) return false;
  return tap_dy<true>(1, cx) == 0 && tap_dx<true>(1) == 0;
}
constexpr bool hex_taps_rule(int cx) {       // the comment above, for a cell in column cx
  const int up = (cx & 1) ? 0 : -1;          // the upper neighbour's row offset in an adjacent column; the lower one's is up + 1
  return tap_dy<true>(0, cx) == -1 && tap_dx<true>(0) == 0 && tap_dy<true>(2, cx) == 1 && tap_dx<true>(2) == 0 &&
         tap_dy<true>(3, cx) == up && tap_dx<true>(3) == -1 && tap_dy<true>(4, cx) == up + 1 && tap_dx<true>(4) == -1 &&
         tap_dy<true>(5, cx) == up && tap_dx<true>(5) == 1 && tap_dy<true>(6, cx) == up + 1 && tap_dx<true>(6) == 1;
}
static_assert(tap_count<false>() == 9 && square_taps_ok(), "square taps");
static_assert(tap_count<true>() == 7 && hex_taps_distinct(0) && hex_taps_distinct(1), "hexagonal taps: seven cells, centre at tap 1");
static_assert(hex_taps_rule(0) && hex_taps_rule(1) && hex_taps_rule(2) && hex_taps_rule(3), "hexagdly's even / odd column rule");

// ---- split-bf16 arithmetic ------------------------------------------------------------------------------------------------
// 8 float32 -> three bf16 pieces (exact: 8 + 8 + 8 significant bits)
__device__ __forceinline__ void split8(const f32x4& lo, const f32x4& hi, u32x4& p0, u32x4& p1, u32x4& p2) {
  const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  uint32_t a[4], b[4], c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float x0 = v[2 * j], x1 = v[2 * j + 1];
    a[j] = pack_hi16(x0, x1);
    const float r0 = x0 - bf16_trunc(x0), r1 = x1 - bf16_trunc(x1);
    b[j] = pack_hi16(r0, r1);
    c[j] = pack_hi16(r0 - bf16_trunc(r0), r1 - bf16_trunc(r1));
  }
  p0 = u32x4{a[0], a[1], a[2], a[3]};
  p1 = u32x4{b[0], b[1], b[2], b[3]};
  p2 = u32x4{c[0], c[1], c[2], c[3]};
}
// one K step (32 channels of one tap): the six piece products, small terms first (net_dev.hpp pair_mfma)
// The weights go in as the MFMA's first operand, so the output tile comes out transposed: lane l holds ROW l & 15 and the
// four consecutive channels 4 (l >> 4) .. + 3 -- one address, one bounds check and three 8-byte stores per lane in the
// epilogue where the other orientation (a column and four rows per lane) needs four of each and twelve 2-byte stores.
__device__ __forceinline__ void step16(f32x4& acc, const u32x4 (&a)[3], const u32x4 (&b)[3]) {
  acc = mfma_bf16(b[1], a[1], acc);
  acc = mfma_bf16(b[0], a[2], acc);
  acc = mfma_bf16(b[2], a[0], acc);
  acc = mfma_bf16(b[0], a[1], acc);
  acc = mfma_bf16(b[1], a[0], acc);
  acc = mfma_bf16(b[0], a[0], acc);
}
// ---- plain-bf16 arithmetic (NZ_PREC_BF16) ----------------------------------------------------------------------------------
// One bf16 per number instead of three: weights, input planes and every stored activation are rounded to nearest even
// ONCE, where the float32 mode splits them; a K step is one MFMA on (stored bf16 activations, bf16 weights) with the same
// float32 accumulator and the same tap / K-group order; the epilogue adds the residual (the stored bf16 value, widened),
// activates as the float32 mode does and stores one bf16 into piece plane 0 of the destination.  Piece planes 1 and 2 of
// a layer's destination are neither written nor read; float32 rows (logits, value plane), the softmax and the value
// are the float32 mode's.  The program, its LDS layout and the weight stream's order ([col tile][tap][32-channel
// group][lane][4], without the piece dimension) are otherwise unchanged.
// (PREC_F32 / PREC_BF16, prec_pieces and pack_rne16: bf16_split.hpp, shared with net_dev.hpp)
// 8 float32 -> 8 bf16 (the input planes, where split8 splits them)
__device__ __forceinline__ u32x4 round8(const f32x4& lo, const f32x4& hi) {
  return u32x4{pack_rne16(lo[0], lo[1]), pack_rne16(lo[2], lo[3]), pack_rne16(hi[0], hi[1]), pack_rne16(hi[2], hi[3])};
}
// one K step: the one product term (weights first, as step16)
__device__ __forceinline__ void step16_bf16(f32x4& acc, const u32x4& a, const u32x4& b) { acc = mfma_bf16(b, a, acc); }

// exp(x) - 1 for x <= 0 to an absolute error of ~1e-7 (v_exp_f32; libm's expm1f keeps the RELATIVE error small near zero,
// thirty instructions the activations' 1e-5 tolerance has no use for)
__device__ __forceinline__ float fast_expm1(float x) { return __expf(x) - 1.0f; }

// ---- the program ----------------------------------------------------------------------------------------------------------
constexpr int FUSED_MAX_OPS = 176;
struct Fused16Op {
  const uint32_t* w;                       // [col tile][tap][32-channel group][piece][lane][4 dwords = 8 bf16] (plain-bf16 mode: no piece dimension)
  int32_t off0, cs0, ps0, kg0;             // source 0: float offset, floats per row and per piece, piece stride, K groups
  int32_t off1, cs1, ps1, kg1;             // source 1 (off1 = -1: none)
  int32_t offd, csd, psd;                  // destination (psd = 0: float32 rows [row][csd])
  int32_t offr, csr, psr;                  // residual (offr = -1: none)
  int32_t ntiles, act;
  int32_t w_lds, w_chunks;                 // 1: weights staged in LDS; 16-byte chunks of one column tile
  int32_t w_slot, w_after_barrier;
  int32_t pad;
};
struct Fused16Program {
  int32_t n_ops, hw, h, wd, planes, hex;
  int32_t zrow_index, lds_floats;           // every pieces buffer has a row of zeros at this index (never written)
  int32_t clear_from, clear2_from;          // LDS floats [clear_from, lds_floats) and [clear2_from, clear2_to) start as zeros:
                                            // the activation buffers (a K group of 32 channels reaches past a layer's last 16)
  int32_t wbuf_off[2];
  int32_t in_off, in_cs, in_ps, pol_off, pol_cs, val_off, val_cs, clear2_to;
  int32_t zero_at_op, n_zero, zero_off[6], zero_len;   // rows of zeros to (re)make before that layer: buffers that take over a weight buffer's space
  // the per-wavefront-pair program (boardnet_wave_program) only: the layers from solo_at on are two independent chains
  // (the policy head's solo_pol layers, then the value head's) that the pair's two wavefronts run side by side; the first
  // chain's hidden buffer has its row of zeros at float offset solo_zero_off (solo_zero_len floats), remade every pass
  int32_t solo_at, solo_pol, solo_zero_off, solo_zero_len;
  Fused16Op ops[FUSED_MAX_OPS];
};

// The header and the layer descriptors reach the scalar registers through VECTOR loads: lane i loads dword i, v_readlane
// makes the scalars when they are wanted.  (As scalar loads they are chains of dependent round trips to memory that come
// back out of order: the first wait for an LDS read behind one waits for memory too.)
constexpr int FUSED16_HDR_DWORDS = (int)(offsetof(Fused16Program, ops) / 4), FUSED16_OP_DWORDS = (int)(sizeof(Fused16Op) / 4);
static_assert(FUSED16_HDR_DWORDS <= 64 && sizeof(Fused16Op) % 4 == 0 && FUSED16_OP_DWORDS <= 64, "one dword per lane");
typedef const __attribute__((address_space(1))) uint32_t* fused16_words;       // global (not flat) loads
// this lane's dword of the header / of layer i's descriptor; zero in the lanes past its end
__device__ __forceinline__ uint32_t fused16_header_dword(const Fused16Program* prog, int lane) {
  return lane < FUSED16_HDR_DWORDS ? ((fused16_words)reinterpret_cast<const uint32_t*>(prog))[lane] : 0u;
}
__device__ __forceinline__ uint32_t fused16_op_dword(const Fused16Program* prog, int i, int lane) {
  return lane < FUSED16_OP_DWORDS ? ((fused16_words)reinterpret_cast<const uint32_t*>(prog->ops))[i * FUSED16_OP_DWORDS + lane] : 0u;
}
// a descriptor out of the register fused16_op_dword filled
__device__ __forceinline__ Fused16Op fused16_unpack(uint32_t v) {
  uint32_t words[FUSED16_OP_DWORDS];
#pragma unroll
  for (int i = 0; i < FUSED16_OP_DWORDS; ++i) words[i] = __builtin_amdgcn_readlane(v, i);
  Fused16Op op;
  __builtin_memcpy(&op, words, sizeof(Fused16Op));
  return op;
}
// a header field out of the register fused16_header_dword filled
#define FUSED16_HDR(hdr_v, field) ((int)__builtin_amdgcn_readlane(hdr_v, (int)(offsetof(::nz::Fused16Program, field) / 4)))

// A layer's K loop is straight-line code for its number of 32-channel K groups: f(std::integral_constant<int, kgt>),
// kgt = 1 .. 4 (the planners admit no more)
template <typename F>
__device__ __forceinline__ void for_kgroups(int kgt, F&& f) {
  if (kgt == 1) f(std::integral_constant<int, 1>{});
  else if (kgt == 2) f(std::integral_constant<int, 2>{});
  else if (kgt == 3) f(std::integral_constant<int, 3>{});
  else f(std::integral_constant<int, 4>{});
}

// ---- the layer epilogue's values: residual, activation, split ---------------------------------------------------------------
// A lane holds four consecutive channels of one row; `q`: the residual's three pieces of those channels, 8 bytes each.
// The pieces add up to the float32 they were split from.
__device__ __forceinline__ void epi16_add_residual(float* v, const uint2& q0, const uint2& q1, const uint2& q2) {
  v[0] += (bf16_lo(q0.x) + bf16_lo(q1.x)) + bf16_lo(q2.x);
  v[1] += (bf16_hi(q0.x) + bf16_hi(q1.x)) + bf16_hi(q2.x);
  v[2] += (bf16_lo(q0.y) + bf16_lo(q1.y)) + bf16_lo(q2.y);
  v[3] += (bf16_hi(q0.y) + bf16_hi(q1.y)) + bf16_hi(q2.y);
}
// Fused16Op::act (0 none, 1 relu, 2 tanh, 3 elu) of N values: they go through the step TOGETHER (one wave-uniform switch,
// then N independent chains the scheduler interleaves)
template <int N>
__device__ __forceinline__ void epi16_activate(float* v, int act) {
  switch (act) {
    case 1:
#pragma unroll
      for (int r = 0; r < N; ++r) v[r] = v[r] > 0.f ? v[r] : 0.f;
      break;
    case 2:
#pragma unroll
      for (int r = 0; r < N; ++r) v[r] = tanhf(v[r]);
      break;
    case 3:
#pragma unroll
      for (int r = 0; r < N; ++r) v[r] = v[r] > 0.f ? v[r] : fast_expm1(v[r]);
      break;
    default: break;
  }
}
// exact three-way split of the four values: q[piece] = the 8 bytes of that piece (v_perm packs two upper halves)
__device__ __forceinline__ void epi16_split(const float* v, uint2 (&q)[3]) {
  float r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = v[i];
#pragma unroll
  for (int piece = 0; piece < 3; ++piece) {
    q[piece] = uint2{pack_hi16(r[0], r[1]), pack_hi16(r[2], r[3])};
    if (piece < 2) {
#pragma unroll
      for (int i = 0; i < 4; ++i) r[i] = r[i] - bf16_trunc(r[i]);
    }
  }
}

// the plain-bf16 mode's residual (`q`: the stored bf16 values of the lane's four channels) and its one-piece store
__device__ __forceinline__ void epi16_add_residual_bf16(float* v, const uint2& q) {
  v[0] += bf16_lo(q.x);
  v[1] += bf16_hi(q.x);
  v[2] += bf16_lo(q.y);
  v[3] += bf16_hi(q.y);
}
__device__ __forceinline__ uint2 epi16_round(const float* v) { return uint2{pack_rne16(v[0], v[1]), pack_rne16(v[2], v[3])}; }

// ---- the two outputs ------------------------------------------------------------------------------------------------------
// Lanes walk the actions i = first, first + stride, ... < A as f(i, cell, plane, j) -- action i = plane * hw + cell, the
// policy planes' layout -- without a division per entry; j = the entry's place in its block of BLOCK entries (a constant
// after unrolling, for callers that keep a register per place).
template <int BLOCK, typename F>
__device__ __forceinline__ void for_each_action_blocked(int A, int hw, int first, int stride, F f) {
  int cell = first % hw, plane = first / hw;
  const int dcell = stride % hw, dplane = stride / hw;
  for (int i0 = first; i0 < A; i0 += stride * BLOCK) {
#pragma unroll
    for (int j = 0; j < BLOCK; ++j) {
      const int i = i0 + stride * j;
      if (i < A) f(i, cell, plane, j);
      cell += dcell; plane += dplane;
      if (cell >= hw) { cell -= hw; ++plane; }
    }
  }
}
template <typename F>
__device__ __forceinline__ void for_each_action(int A, int hw, int first, int stride, F f) {
  for_each_action_blocked<1>(A, hw, first, stride, [&](int i, int cell, int plane, int) { f(i, cell, plane); });
}
// The order of the softmax sum over a position's exp(logit - max): each of `ways` partial sums takes every (64 x ways)-th
// entry per lane (partial sum s of lane l: entries 64 s + l, + 64 ways, ...), one butterfly over the wavefront per partial
// sum, the partial sums added in index order.  fused16_net_kernel gives a position `ways` of its sixteen wavefronts, by
// the positions its workgroup holds; persist_leader forms the same partial sums on one wavefront.
__host__ __device__ constexpr int softmax_ways(int positions_per_workgroup) {
  return positions_per_workgroup <= 4 ? 4 : (positions_per_workgroup <= 8 ? 2 : 1);
}
__device__ __forceinline__ float wave_sum(float x) {
  for (int w = 32; w; w >>= 1) x += __shfl_xor(x, w, 64);
  return x;
}
// value = tanh(mean of the value plane) (blocks.py:82-84); `lane_sum`: this lane's cells c = lane, lane + 64, ... added up
__device__ __forceinline__ float value_of_plane(float lane_sum, int hw) { return tanhf(wave_sum(lane_sum) / (float)hw); }

}  // namespace nz
