// The packed pass: the fused policy/value network of net_dev.hpp for P <= NET_PACKED_MAX positions per workgroup.
//
// net_tile's MFMA columns are 16 positions; a persistent engine of a few hundred games plays one to eight games per
// workgroup and multiplies 16 columns all the same.  Here the columns are the live (position, cell) pairs: pair
// c = 9 pos + cell is column c % 16 of column tile c / 16, T = ceil(9 P / 16) tiles in all.  For one tap the weights (the
// A operand) are the same for every column, and a column's activation fragment (the B operand) is that of input cell
// cell + (dy, dx) of its position -- all zeros where that cell is off the board, and in the 16 T - 9 P dead columns.
// Per 32-channel K group and 16-channel output tile that is 9 T chains of six MFMAs (9, 18, 18, 27, 27, 36, 36, 45 for
// P = 1 .. 8) where net_tile issues 49.
//
// Arithmetic.  Bit for bit net_tile's: a column is one output element's (position, cell), and its accumulator takes K
// groups ascending, inside a K group taps 0 .. 8 ascending, per tap pair_mfma's six piece products, then the input
// planes' float32 MFMA steps in tap order, then epi_step's steps; the value is net_value_mean's.  A tap that is off the
// board for a column issues with a zero fragment: the accumulator starts at +0, and adding sums of +-0 products leaves
// its bits alone.  The chain, the input-plane step and the epilogue steps are net_dev.hpp's own functions, called for
// the one-cell group {4}: through tap t the centre cell reads "input cell" t, so a column's fragment for tap t is
// handed over as input cell t.
//
// Layout.  The two activation buffers' bytes hold four AREAS of 9 P <= 72 rows, row = 9 pos + cell, 64 channels (128
// bytes) a row in each of the three bf16 pieces: area a is rows 72 (a >> 1) .. of buffer a & 1, pieces PIECE_BYTES apart
// as in net_tile's layout (epi_step's stores apply unchanged).  The 16-byte slot index is rotated by 2 (row >> 1): the
// columns of a tile read consecutive rows (a tap shifts them all by 3 dy + dx), and a ds_read_b128 lane group is eight
// lanes of one quad on rows r .. r + 3, r + 12 .. r + 15 and eight of the next quad on rows r + 4 .. r + 11.  Rows 2 k
// and 2 k + 1 share a slot in the two halves of the 256-byte bank window; the first quad's row pairs k, k + 1, k + 6,
// k + 7 land on the four even rotations, the second quad's k + 2 .. k + 5, one slot on, on the four odd ones: sixteen
// different slots whatever the tap's shift (the XOR swizzle of net_tile's slot_addr collides for odd shifts).  The
// epilogue's ds_write_b64, far fewer, pay a four-way conflict for it.  With four
// areas the heads need no strip: the policy head's first conv writes an area of its own.  The strip's bytes stay zero
// and are where the fragments of off-board taps are read from (PK_ZEROS).
//
// Work split (engine.hip compile_net_packed).  A job is one (conv, output tile, run of up to NET_PACKED_RUN column
// tiles): the weights of a tap are read once per job and used for every column tile of the run.  The jobs of a stage are
// dealt to the eight waves longest first; the weight stream runs three taps ahead as in net_tile, the operand fragments
// one tap ahead.
#pragma once
#include "net_dev.hpp"

namespace nz {

constexpr int PK_ROWS = 9 * NET_PACKED_MAX;       // rows of an area
constexpr int PK_GROUP = 0x010;                   // the one-cell group {4}: tap t reaches it from "input cell" t
static_assert(2 * PK_ROWS * 128 <= PIECE_BYTES, "two areas in one buffer's piece");
// Sixteen bytes of zeros for the fragments of off-board taps: the start of net_tile's strip, which the callers zero
// with the buffers and the packed pass never writes.
constexpr int PK_ZEROS = (NET_LDS_FLOATS - STRIP_FLOATS) * 4;
static_assert(PK_ZEROS % 16 == 0 && STRIP_FLOATS >= 4, "an aligned 16-byte read inside the strip");
static_assert(TapMap<0, 0>::o == 4 && TapMap<3, 3>::o == 4 && TapMap<8, 8>::o == 4 && pairs_before(PK_GROUP, 9, 0) == 9,
              "tap t, input cell t -> the centre cell");

// byte offset of area `area` (piece 0) in the activation buffers
__device__ __forceinline__ int pk_area(int area) { return (area & 1) * ACT_BYTES + (area >> 1) * (PK_ROWS * 128); }
// byte offset of the 16-byte slot holding channels 8 s .. 8 s + 7 of `row` inside one piece of an area
__device__ __forceinline__ int pk_slot(int row, int s) { return (row << 7) + (((s + (row & ~1)) & 7) << 4); }

// this lane's column of column tile `tile`: pair index, liveness, cell coordinates
struct PkColumn {
  int c, y, x;
  bool live;
};
__device__ __forceinline__ PkColumn pk_column(int tile, int lane, int P) {
  PkColumn k;
  k.c = tile * 16 + (lane & 15);
  k.live = k.c < 9 * P;
  const int cell = k.c % 9;
  k.y = cell / 3;
  k.x = cell - 3 * k.y;
  return k;
}
// whether tap TAP of the column is on the board, and the row it then reads
template <int TAP>
__device__ __forceinline__ bool pk_tap_on(const PkColumn& k) {
  constexpr int dy = TAP / 3 - 1, dx = TAP % 3 - 1;
  return k.live && (unsigned)(k.y + dy) < 3u && (unsigned)(k.x + dx) < 3u;
}
template <int TAP>
__device__ __forceinline__ int pk_tap_row(const PkColumn& k) {
  constexpr int dy = TAP / 3 - 1, dx = TAP % 3 - 1;
  return k.c + 3 * dy + dx;
}

// The fragments of tap TAP, K-group slot `s` (first slot + quad), for the NT column tiles of the job: as input cell TAP.
// `src`: byte offset of the source area in `lds`.  A tap that is off the board reads PK_ZEROS for all three pieces: the
// choice is made on the address, so nothing waits for the data before the MFMA that uses it.
template <int NT, int TAP>
__device__ __forceinline__ void pk_load(Operands<PK_GROUP> (&xs)[NT], const PkColumn (&col)[NT],
                                        const unsigned char* __restrict__ lds, int src, int s) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const bool on = pk_tap_on<TAP>(col[t]);
    const int a = src + pk_slot(pk_tap_row<TAP>(col[t]), s);
#pragma unroll
    for (int piece = 0; piece < 3; ++piece)
      xs[t].x[TAP].p[piece] = *reinterpret_cast<const u32x4*>(lds + (on ? a + piece * PIECE_BYTES : PK_ZEROS));
  }
}
// Step S of a job's K loop: tap S % 9 of K group S / 9.  The fragments of the step after the next are requested first
// (PK_AHEAD steps ahead: a one-tile job's tap is six MFMAs, shorter than an LDS read's way back), then this step's chains
// issue (one per column tile, the same weights), then the ring slot takes the tap three steps on -- of this job's
// stream, or of the next job's (`w_after`; any readable weights when nothing follows).
constexpr int PK_AHEAD = 2;
template <int NT, int KG, int S>
__device__ __forceinline__ void pk_steps(f32x4 (&acc)[NT][CELLS], Operands<PK_GROUP> (&xs)[NT], const PkColumn (&col)[NT],
                                         FragS& f, const unsigned char* __restrict__ lds, int src, int s0,
                                         const float* __restrict__ w, const float* __restrict__ w_after, int lane) {
  if constexpr (S < 9 * KG) {
    constexpr int TAP = S % 9;
    if constexpr (S + PK_AHEAD < 9 * KG) pk_load<NT, (S + PK_AHEAD) % 9>(xs, col, lds, src, s0 + 4 * ((S + PK_AHEAD) / 9));
    NoEpi none;
#pragma unroll
    for (int t = 0; t < NT; ++t) pair_mfma<PK_GROUP, TAP, TAP, 0>(acc[t], xs[t], f.rb[TAP % W_RING], none);
    load_tap(f.rb[TAP % W_RING], S + W_RING < 9 * KG ? w + (S + W_RING) * TAP_DWORDS : w_after + (S + W_RING - 9 * KG) * TAP_DWORDS, lane);
    pk_steps<NT, KG, S + 1>(acc, xs, col, f, lds, src, s0, w, w_after, lane);
  }
}
template <int NT, int KG>
__device__ __forceinline__ void pk_kloop(f32x4 (&acc)[NT][CELLS], const PkColumn (&col)[NT], FragS& f,
                                         const unsigned char* __restrict__ lds, int src, int sslot,
                                         const float* __restrict__ w, const float* __restrict__ w_after, int lane) {
  static_assert(W_RING == 3 && 9 % W_RING == 0, "a tap's ring slot does not depend on its K group");
  static_assert(PK_AHEAD == 2, "the steps requested before the loop");
  Operands<PK_GROUP> xs[NT];
  const int s0 = sslot + (lane >> 4);
  pk_load<NT, 0>(xs, col, lds, src, s0);
  pk_load<NT, 1>(xs, col, lds, src, s0);
  pk_steps<NT, KG, 0>(acc, xs, col, f, lds, src, s0, w, w_after, lane);
}

// the input planes' step (extra_planes): the column's plane values of tap t's source cell as input cell t
template <int TAP>
__device__ __forceinline__ void pk_plane_taps(f32x4 (&acc)[CELLS], float (&ax)[CELLS], const float (&bx)[9],
                                              const PkColumn& k, const __attribute__((address_space(3))) float* inl, int lane) {
  if constexpr (TAP < 9) {
    const bool on = pk_tap_on<TAP>(k);
    const int row = on ? pk_tap_row<TAP>(k) : 0, pos = row / 9, cell = row - 9 * pos;
    const float v = inl[(cell * POS + pos) * 4 + (lane >> 4)];
    ax[TAP] = on ? v : 0.0f;
    mfma_extra_tap<PK_GROUP, TAP>(acc, ax, bx);
    pk_plane_taps<TAP + 1>(acc, ax, bx, k, inl, lane);
  }
}
template <int NT>
__device__ __forceinline__ void pk_extra_planes(f32x4 (&acc)[NT][CELLS], const PkColumn (&col)[NT],
                                                const float* __restrict__ wx, const float* __restrict__ inp, int lane) {
  float bx[9];
  const __attribute__((address_space(1))) float* wxg = (const __attribute__((address_space(1))) float*)wx;
  const __attribute__((address_space(3))) float* inl = (const __attribute__((address_space(3))) float*)inp;
#pragma unroll
  for (int t = 0; t < 9; ++t) bx[t] = wxg[t * 64 + lane];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    float ax[CELLS];
    pk_plane_taps<0>(acc[t], ax, bx, col[t], inl, lane);
  }
}

// ---- epilogue: lane holds C[cout = 16 nt + 4 quad + r][column] -- four channels of its column's row ------------------
template <int ACT, bool RES>
__device__ __forceinline__ void pk_epilogue_row(const f32x4& a, const PkColumn& k, unsigned char* __restrict__ dst,
                                                const unsigned char* res, int lane, int dtile) {
  if (k.live) {                                     // a dead column has no row
    const int quad = lane >> 4;
    const int off = pk_slot(k.c, dtile * 2 + (quad >> 1)) + (quad & 1) * 8;
    u32x2 q[3];
    if constexpr (RES) epi_read_res<0>(q, res, off);
    epilogue_cell<0, ACT, RES, false>(a, q, dst, off);
  }
}
template <int NT>
__device__ __forceinline__ void pk_epilogue(const f32x4 (&acc)[NT][CELLS], const PkColumn (&col)[NT], const NetJob& job,
                                            unsigned char* __restrict__ lds, int lane, int policy_channels, int n_valid,
                                            float* logits, float* vcells) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const f32x4& a = acc[t][4];
    const PkColumn& k = col[t];
    if (job.dst < NET_PACKED_AREAS) {
      unsigned char* dst = lds + pk_area(job.dst);
      if (job.res >= 0) pk_epilogue_row<1, true>(a, k, dst, lds + pk_area(job.res), lane, job.dtile);
      else if (job.act == 1) pk_epilogue_row<1, false>(a, k, dst, nullptr, lane, job.dtile);
      else if (job.act == 2) pk_epilogue_row<2, false>(a, k, dst, nullptr, lane, job.dtile);
      else if (job.act == 3) pk_epilogue_row<3, false>(a, k, dst, nullptr, lane, job.dtile);
      else pk_epilogue_row<0, false>(a, k, dst, nullptr, lane, job.dtile);
    } else {
      const int pos = k.c / 9, cell = k.c - 9 * pos, quad = lane >> 4;
      if (job.dst == NET_PACKED_DST_POLICY) {       // policy logits [pos][P][9]
        if (k.live && pos < n_valid) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int cout = job.nt * 16 + quad * 4 + r;
            if (cout < policy_channels) logits[((size_t)pos * policy_channels + cout) * CELLS + cell] = a[r];
          }
        }
      } else if (k.live && job.nt == 0 && quad == 0) {   // value: channel 0 of every cell, for net_value_mean
        vcells[cell * POS + pos] = a[0];
      }
    }
  }
}

// one job: K loop, input-plane step, epilogue
template <int NT, typename Fetch>
__device__ __forceinline__ void pk_run_job(const NetJob& job, int P, FragS& f, const float* __restrict__ W,
                                           const float* w_after, unsigned char* __restrict__ lds,
                                           const float* __restrict__ inp, int lane, int policy_channels, int n_valid,
                                           float* logits, float* vcells, Fetch&& fetch_next) {
  asm volatile("" : "+v"(lane));                  // per-lane addresses are derived inside the job (net_dev.hpp run_job_plain)
  PkColumn col[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) col[t] = pk_column((job.og & 7) + t, lane, P);
  f32x4 acc[NT][CELLS];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t][4] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (job.kgroups == 2) pk_kloop<NT, 2>(acc, col, f, lds, pk_area(job.src), job.sslot, W + job.w_off, w_after, lane);
  else if (job.kgroups == 1) pk_kloop<NT, 1>(acc, col, f, lds, pk_area(job.src), job.sslot, W + job.w_off, w_after, lane);
  if (job.extra) pk_extra_planes<NT>(acc, col, W + job.wx_off, inp, lane);
  fetch_next();
  pk_epilogue<NT>(acc, col, job, lds, lane, policy_channels, n_valid, logits, vcells);
}

// Run the packed program `prog` (compiled for P) on the P positions whose input planes are in `inp` ([cell][pos][4
// planes], pos < P); `lds_f` as for net_tile: the activation buffers (no NaN bit patterns: the callers zero them once),
// then `inp`, then the value staging, then the strip (zeroed once as well, never written here).  Every thread of the workgroup must call it; it ends with a workgroup barrier.
// Outputs: logits [pos][policy_channels][9] and value [pos] for pos < n_valid <= P (any address space).
__device__ __forceinline__ void net_tile_packed(const NetProgram* __restrict__ prog, const float* __restrict__ W,
                                                float* __restrict__ lds_f, const float* __restrict__ inp, int P,
                                                int policy_channels, int n_valid, float* logits, float* value) {
  unsigned char* __restrict__ lds = reinterpret_cast<unsigned char*>(lds_f);
  float* const vcells = lds_f + NET_BUFFERS * ACT_FLOATS + INP_FLOATS;
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const NetJob* __restrict__ jobs = prog->jobs[wave];
  const int n_jobs = __builtin_amdgcn_readfirstlane(prog->n_jobs[wave]);
  const int first_w = __builtin_amdgcn_readfirstlane(prog->first_w_off[wave]);
  P = __builtin_amdgcn_readfirstlane(P);

  FragS f;
  zero_b(f);
  if (first_w >= 0) load_b(f, W + first_w, lane);

  // the next job's descriptor travels as in net_tile: vector loads under the epilogue, scalars again by v_readfirstlane
  static_assert(sizeof(NetJob) == 24, "six dwords");
  int vzero;
  asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
  const __attribute__((address_space(1))) uint32_t* jw =
      (const __attribute__((address_space(1))) uint32_t*)reinterpret_cast<const uint32_t*>(jobs) + vzero;
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
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) only: the ring's loads are an epilogue old (net_tile)
    auto fetch_next = [&]() {
      if (j + 1 < n_jobs) {
#pragma unroll
        for (int i = 0; i < 6; ++i) nw[i] = jw[(j + 1) * 6 + i];
      }
    };
    if (job.og == OG_NONE) {
      fetch_next();
    } else {
      const float* w_after = W + (job.next_w_off >= 0 ? job.next_w_off : 0);
      switch (job.og >> 3) {
        case 1: pk_run_job<1>(job, P, f, W, w_after, lds, inp, lane, policy_channels, n_valid, logits, vcells, fetch_next); break;
        default: pk_run_job<2>(job, P, f, W, w_after, lds, inp, lane, policy_channels, n_valid, logits, vcells, fetch_next); break;
      }
      static_assert(NET_PACKED_RUN == 2, "the runs compiled in");
    }
    if (job.flags & NET_JOB_STAGE_END) __syncthreads();
  }
  net_value_mean(lds_f, tid, n_valid, value);
  __syncthreads();
}

}  // namespace nz
