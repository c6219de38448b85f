// Host side of the C ABI (include/nuzero_amd.h): buffer ownership, the per-move
// launch sequence, weight packing for the MFMA kernel and the host random
// streams' call order.  No compute happens here.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "engine.h"
#include "hip_own.hpp"
#include "scs_mt.hpp"
#include "ttt_agents.hpp"
#include "weight_pack.hpp"

using namespace nz;

namespace {
thread_local std::string g_create_error;

struct ProfileSpan {
  Event a, b;
  int cls = 0;
};

// The device arrays made by nz_engine_create, one owner each: TreeParams and the launches borrow their pointers.
struct EngineArrays {
  DevBuf<TNode> nodes;
  DevBuf<uint32_t> board, leaf_board, leaf_boards, hist_board;
  DevBuf<uint32_t> start_board;                 // [G] nz_engine_reset_to's positions, made at its first call
  DevBuf<int32_t> next_game, length, alive, outcome, root, node_count, sims_left, pending, path, path_len, sim_count, exp_count,
      sel_nodes, sel_children, new_nodes, n_root_children, desync, leaf_count, error_flag, hist_action, hist_visits,
      hist_tree_size, hist_children;
  DevBuf<float> leaf_logits, leaf_value;
  DevBuf<double> bias_tab, sqrt_tab, hist_bias, hist_prior, hist_value_sum, hist_root_value_sum;
  DevBuf<double> noise, uniforms, game_noise, game_uniforms;   // one move's randomness [G][A], [G][3]; a whole game's [G][T]...
  DevBuf<unsigned long long> stamps;          // [blocks][4], diagnostic build only
  DevBuf<NetProgram> prog;
};

// The state of the evaluation matches of nz_engine_match_play (ttt_agents.hpp), made at the first round and owned by
// the round's first engine; TttMatchArgs borrows the pointers.
struct MatchArrays {
  DevBuf<uint32_t> board, start, mt_keys[2], seeds[2];
  DevBuf<int32_t> alive, length, outcome, actions, forced, err, agent_actions[2], agent_n_legal[2], mt_pos[2];
  DevBuf<float> states, logits, value, probs;
  DevBuf<unsigned long long> tally;           // [8]
  PinnedBuf<unsigned long long> h_tally;      // [8]
  bool ensure(size_t n) {
    const size_t nt = n * TTT_MAX_MOVES;
    bool ok = board.ensure(n) && start.ensure(n) && alive.ensure(n) && length.ensure(n) && outcome.ensure(n) && actions.ensure(nt) &&
              forced.ensure(n) && err.ensure(n) && states.ensure(n * 18) && logits.ensure(n * TTT_ACTIONS) &&
              value.ensure(n) && probs.ensure(n * TTT_ACTIONS) && tally.ensure(8) && h_tally.ensure(8);
    for (int s = 0; s < 2; ++s)
      ok = ok && agent_actions[s].ensure(nt) && agent_n_legal[s].ensure(nt) && mt_keys[s].ensure(n * MT_N) &&
           mt_pos[s].ensure(n) && seeds[s].ensure(n);
    return ok;
  }
};

// Where pack_conv (below) put one conv tensor's streams, and the shape they were packed for.
struct PackedConv {
  int cout, cin, cin_main, kgroups, ntiles, extra;
  int32_t w_off, wx_off;
  int kg_dwords;       // dwords of one K group of one output tile in the stream: NET_KG_DWORDS, or NET_KG_DWORDS_BF16
};
}  // namespace

struct nz_engine {
  nz_search_cfg cfg;
  nz_game_desc game;
  int device = 0;
  int n_games = 0;   // games per round
  int n_slots = 0;   // games in flight
  int cap = 0;
  int tab_len = 0;
  TreeParams tp;
  EngineArrays dev;
  std::string error;
  // network
  bool have_net = false, have_table = false;
  nz_net_desc net;
  int iters = 0;
  NetProgram prog_host;
  // the packed pass (net_packed_dev.hpp): whether nz_engine_play's kernel takes it (decided at create), and the
  // programs compiled so far for the current weights, by positions per pass (packed_program below)
  bool packed = false;
  // the arithmetic mode (nz_engine_precision).  NZ_PREC_BF16 exists for the 16-column pass on a wave's own job list
  // only: `packed` and tp.burst_under_net are off while it holds, and what nz_engine_create chose for float32 waits here
  int prec = NZ_PREC_FLOAT32;
  bool f32_packed = false;
  int f32_burst = 0, f32_sims_per_cycle = 0;
  std::vector<PackedConv> convs;              // the packed tensors' layout, as nz_engine_set_weights made it
  DevBuf<NetProgram> packed_prog[NZ_NET_PACKED_MAX + 1];
  bool packed_ready[NZ_NET_PACKED_MAX + 1] = {};
  DevBuf<float> weights_dev, table_dev;
  const float* borrowed_weights = nullptr;    // fallback engine: the parent's packed weights, used instead of weights_dev
  double executed_bf16_flops_per_position = 0.0, executed_f32_flops_per_position = 0.0;
  double algorithmic_flops_per_position = 0.0;
  // host staging for nz_engine_play
  PinnedBuf<int32_t> h_children, h_alive, h_desync;   // [G]
  PinnedBuf<double> h_noise, h_uniforms;    // [G][A], [G][3]
  std::vector<nz_rng*> rngs;
  // persistent-kernel path: whole-game randomness, [G][T][A] and [G][T][3]
  PinnedBuf<double> h_game_noise, h_game_uniforms;
  // randomness of the NEXT round, drawn on host threads while this round's kernel runs (nz_engine_play_next)
  PinnedBuf<double> h_next_noise, h_next_uniforms;   // [G][T][A], [G][T][3]
  bool next_ready = false;
  uint64_t next_seed = 0;
  nz_engine* fallback = nullptr;
  int64_t desync_total = 0;
  bool stamps = false;
  // profiling
  bool profile = false;
  std::vector<ProfileSpan> spans;
  int64_t net_positions = 0;       // upper bound: positions offered to the network kernel
  // evaluation matches (nz_engine_match_play)
  MatchArrays match;
  int match_kinds[2] = {-1, -1};   // the last round's sides, -1: none played
};

namespace {

nz_status fail(nz_engine* e, nz_status code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (e) e->error = buf;
  else g_create_error = buf;
  return code;
}

#define NZ_HIP(e, call)                                                                          \
  do {                                                                                           \
    hipError_t err__ = (call);                                                                   \
    if (err__ != hipSuccess)                                                                     \
      return fail((e), NZ_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(err__), __FILE__, __LINE__); \
  } while (0)

const float* net_weights(const nz_engine* e) { return e->borrowed_weights ? e->borrowed_weights : e->weights_dev.get(); }

struct Span {
  nz_engine* e;
  hipStream_t s;
  ProfileSpan sp{};
  bool on;
  Span(nz_engine* e_, hipStream_t s_, int cls) : e(e_), s(s_), on(e_->profile) {
    if (!on) return;
    sp.cls = cls;
    if (!sp.a.create() || !sp.b.create()) { on = false; return; }
    (void)hipEventRecord(sp.a.get(), s);
  }
  ~Span() {
    if (!on) return;
    (void)hipEventRecord(sp.b.get(), s);
    e->spans.push_back(std::move(sp));
  }
};

// One conv tensor repacked for the MFMA kernel (net_dev.hpp): per 16-channel output
// tile nt a contiguous weight stream main[nt][kgroup of 32 ch][tap][piece][lane][8 bf16] (the
// three exact bf16 pieces of every weight) and, for the two convs that also read the raw
// input planes, extra[nt][tap][lane] in float32.
// prec NZ_PREC_BF16 (the plain-bf16 mode; the only stream built in that mode): every weight rounded once to nearest
// even (weight_pack.hpp bf16_rne), the main stream without the piece dimension, main[nt][kgroup][tap][lane][8 bf16], and
// the input-plane weights the rounded values as float32.
// (struct PackedConv: above, the engine keeps the layout)
PackedConv pack_conv(const float* w, int cout, int cin, int cin_main, std::vector<float>& out, int prec = NZ_PREC_FLOAT32) {
  const bool plain = prec == NZ_PREC_BF16;
  PackedConv pc{};
  pc.kg_dwords = plain ? NET_KG_DWORDS_BF16 : NET_KG_DWORDS;
  pc.cout = cout; pc.cin = cin; pc.cin_main = cin_main;
  pc.ntiles = (cout + 15) / 16;
  pc.kgroups = (cin_main + NET_KG_CHANNELS - 1) / NET_KG_CHANNELS;
  pc.extra = cin > cin_main ? 1 : 0;
  while (out.size() % 4) out.push_back(0.f);
  pc.w_off = (int32_t)out.size();
  auto weight = [&](int co, int ci, int t) { return co < cout && ci < cin_main ? w[((size_t)co * cin + ci) * 9 + t] : 0.f; };
  for (int nt = 0; nt < pc.ntiles; ++nt)
    for (int kg = 0; kg < pc.kgroups; ++kg)
      for (int t = 0; t < 9; ++t)
        for (int piece = 0; piece < (plain ? 1 : 3); ++piece)
          for (int lane = 0; lane < 64; ++lane)
            for (int pr = 0; pr < 4; ++pr) {       // lane holds channels 32 kg + 8 (lane >> 4) + 0..7 as 4 bf16 pairs
              const int co = nt * 16 + (lane & 15), ci = kg * 32 + (lane >> 4) * 8 + 2 * pr;
              uint32_t word[3];
              if (plain) word[0] = (uint32_t)bf16_rne(weight(co, ci, t)) | ((uint32_t)bf16_rne(weight(co, ci + 1, t)) << 16);
              else split3_pair(weight(co, ci, t), weight(co, ci + 1, t), word);
              float f;
              memcpy(&f, &word[piece], 4);
              out.push_back(f);
            }
  pc.wx_off = (int32_t)out.size();
  if (pc.extra)
    for (int nt = 0; nt < pc.ntiles; ++nt)
      for (int t = 0; t < 9; ++t)
        for (int lane = 0; lane < 64; ++lane) {
          const int co = nt * 16 + (lane & 15);
          const int ci = cin_main + (lane >> 4);
          float v = co < cout && ci < cin ? w[((size_t)co * cin + ci) * 9 + t] : 0.f;
          if (plain) {
            const uint32_t bits = (uint32_t)bf16_rne(v) << 16;
            memcpy(&v, &bits, 4);
          }
          out.push_back(v);
        }
  return pc;
}

// A stage of the network = convs that may run side by side.  Its units (conv, output tile,
// output-cell group) are dealt to the eight waves longest-first; every wave's last job of the
// stage carries the barrier.
struct StageConv {
  int tensor, src, dst, res, act;
  bool split;      // each output tile may be cut into output-cell groups (halves or quarters) to give every wave a unit
  int sslot = 0;   // first 16-byte slot of the K groups in the source rows, or NET_SSLOT_SPLIT (net_dev.hpp)
  int dtile = 0;   // destination tile of output tile 0 (dst a buffer): tiles past the fourth go to the strip
};
const int og_taps[7] = {49, 13, 12, 12, 12, 26, 23};   // (input cell, tap) pairs per output-cell group (net_dev.hpp og_mask)
const int BURST_LONG_STAGE = 160;   // add_stage cost units from which a stage counts as long for the burst budget
const int JOB_OVERHEAD = 12;   // a job's epilogue and start-up beyond its MFMAs, in the cost units of add_stage (32 cycles)
// `tensor_of[w]` (optional): the conv tensor of every job appended to pg.jobs[w], -1 for a barrier-only job.
bool add_stage(NetProgram& pg, const std::vector<PackedConv>& convs, const std::vector<StageConv>& stage,
               std::vector<int>* tensor_of = nullptr) {
  struct Unit { NetJob job; int cost; int tensor; };
  struct Tile { const StageConv* sc; int nt; };
  std::vector<Tile> tiles;
  for (const StageConv& sc : stage) {
    const PackedConv& pc = convs[sc.tensor];
    if (!sc.split || pc.ntiles >= NET_WAVES_HOST) return false;   // whole-tile jobs (group 0) are not compiled in
    for (int nt = 0; nt < pc.ntiles; ++nt) tiles.push_back({&sc, nt});
  }
  // the units of the stage when the tiles in `quarters` (a bit mask) are cut in four and the others in two
  auto make_units = [&](unsigned quarters, std::vector<Unit>& units) {
    units.clear();
    for (size_t t = 0; t < tiles.size(); ++t) {
      const StageConv& sc = *tiles[t].sc;
      const PackedConv& pc = convs[sc.tensor];
      const int nt = tiles[t].nt;
      const bool q = (quarters >> t) & 1;
      for (int og = q ? 1 : 5; og <= (q ? 4 : 6); ++og) {
        NetJob j{};
        j.w_off = pc.w_off + nt * pc.kgroups * pc.kg_dwords;
        j.wx_off = pc.wx_off + nt * 9 * 64;
        j.kgroups = (int8_t)pc.kgroups;
        j.sslot = (int8_t)sc.sslot;
        j.nt = (int16_t)nt;
        j.extra = (int8_t)pc.extra;
        j.og = (int8_t)og;
        j.src = (int8_t)sc.src; j.dst = (int8_t)sc.dst; j.res = (int8_t)sc.res; j.act = (int8_t)sc.act;
        j.dtile = (int8_t)(sc.dtile + nt);
        if (sc.dst < NET_ACT_BUFFERS && j.dtile >= 4) { j.dst = NET_DST_STRIP; j.dtile = (int8_t)(j.dtile - 4); }
        // ~time in units of 32 cycles (of the float32 mode; the plain-bf16 mode keeps its job lists)
        units.push_back({j, og_taps[og] * (3 * pc.kgroups + pc.extra) + JOB_OVERHEAD, sc.tensor});
      }
    }
    std::stable_sort(units.begin(), units.end(), [](const Unit& a, const Unit& b) { return a.cost > b.cost; });
  };
  auto deal = [](const std::vector<Unit>& units, int (&load)[NET_WAVES_HOST], int* who) {
    for (int w = 0; w < NET_WAVES_HOST; ++w) load[w] = 0;
    for (size_t u = 0; u < units.size(); ++u) {
      int w = 0;
      for (int i = 1; i < NET_WAVES_HOST; ++i)
        if (load[i] < load[w]) w = i;
      load[w] += units[u].cost;
      if (who) who[u] = w;
    }
  };
  // A one-conv stage cuts its tiles in two when that gives every wave a unit, else in four.  A stage of several convs
  // (the two heads side by side) tries every cut of its tiles in halves or quarters and keeps the one whose most loaded
  // matrix pipe (waves w and w + 4 share one SIMD), then whose most loaded wave, has the least work.
  unsigned best = 2 * tiles.size() >= (size_t)NET_WAVES_HOST ? 0u : (1u << tiles.size()) - 1u;
  std::vector<Unit> units;
  if (stage.size() > 1) {
    long best_key = -1;
    for (unsigned m = 0; m < (1u << tiles.size()); ++m) {
      int load[NET_WAVES_HOST];
      make_units(m, units);
      deal(units, load, nullptr);
      int simd = 0, wave = 0;
      for (int w = 0; w < NET_WAVES_HOST; ++w) wave = std::max(wave, load[w]);
      for (int w = 0; w < NET_WAVES_HOST / 2; ++w) simd = std::max(simd, load[w] + load[w + NET_WAVES_HOST / 2]);
      const long key = (long)simd * 65536 + wave;
      if (best_key < 0 || key < best_key) { best_key = key; best = m; }
    }
  }
  make_units(best, units);
  for (const Unit& u : units) {
    if (u.job.dst == NET_DST_STRIP && (u.job.dtile != 0 || u.job.act != 1 || u.job.res >= 0)) return false;
    if (u.job.sslot == NET_SSLOT_SPLIT && u.job.kgroups != 1) return false;
  }
  // Progressive epilogue (NET_JOB_PROGRESSIVE, net_dev.hpp ProgEpi): the job writes an output cell's rows while its own K
  // loop, and the other jobs' of the stage, still read MFMA operands.  Hazard rule: allowed only if no job of the stage
  // reads an area the job writes -- areas are the activation buffers and the strip; a K loop reads its source buffer
  // (and the strip for NET_SSLOT_SPLIT).  The residual is no operand: it is read by the wave that writes those very
  // channels and cells, in program order, so residual blocks qualify (their source is the other buffer).  The kernel
  // has the form for ReLU (with or without residual) and tanh into a buffer, for K loops without the input-plane step
  // (whose MFMAs come after the last tap), and for the groups of net_og_progressive; policy and value
  // outputs, the strip, ELU and everything else keep the end-of-job epilogue.
  unsigned read_areas = 0;   // bit b: buffer b; bit NET_ACT_BUFFERS: the strip
  for (const Unit& u : units) {
    if (u.job.kgroups > 0) read_areas |= 1u << u.job.src;
    if (u.job.sslot == NET_SSLOT_SPLIT) read_areas |= 1u << NET_ACT_BUFFERS;
  }
  for (Unit& u : units) {
    NetJob& j = u.job;
    const bool form = j.dst >= 0 && j.dst < NET_ACT_BUFFERS && j.kgroups >= 1 && !j.extra && j.sslot != NET_SSLOT_SPLIT &&
                      net_og_progressive(og_mask(j.og)) && (j.res >= 0 ? j.act == 1 : (j.act == 1 || j.act == 2));
    if (form && !((read_areas >> j.dst) & 1)) j.flags |= NET_JOB_PROGRESSIVE;
  }
  int load[NET_WAVES_HOST];
  std::vector<int> who(units.size());
  deal(units, load, who.data());
  int first[NET_WAVES_HOST];
  for (int w = 0; w < NET_WAVES_HOST; ++w) first[w] = pg.n_jobs[w];
  for (size_t u = 0; u < units.size(); ++u) {
    const int w = who[u];
    if (pg.n_jobs[w] >= NET_MAX_JOBS) return false;
    pg.jobs[w][pg.n_jobs[w]++] = units[u].job;
    if (tensor_of) tensor_of[w].push_back(units[u].tensor);
  }
  for (int w = 0; w < NET_WAVES_HOST; ++w) {
    if (pg.n_jobs[w] == first[w]) {            // nothing to do in this stage: barrier only
      if (pg.n_jobs[w] >= NET_MAX_JOBS) return false;
      NetJob j{};
      j.og = OG_NONE;
      pg.jobs[w][pg.n_jobs[w]++] = j;
      if (tensor_of) tensor_of[w].push_back(-1);
    }
    pg.jobs[w][pg.n_jobs[w] - 1].flags |= NET_JOB_STAGE_END;
  }
  // the stage's length in the cost model above (compile_net turns it into the stage's simulation budget)
  if (pg.n_stages >= NET_MAX_JOBS) return false;
  int longest = 0;
  for (int w = 0; w < NET_WAVES_HOST; ++w) longest = std::max(longest, load[w]);
  pg.stage_budget[pg.n_stages++] = longest;
  return true;
}

// The list wave p walks in a pass that wave p ^ 4 sits out (NetProgram::solo_jobs): stage by stage p's jobs and then
// p ^ 4's, one barrier after both.  Where the two lists' jobs of a stage are the two cell halves (groups 5 and 6) of
// one tile of one conv into an activation buffer -- the same weights, K groups, source, destination, residual,
// activation and input-plane step -- and `whole_tile` is set, ONE job of group 0 replaces them: one start-up, one weight
// stream and one uncovered tail where the two jobs, alone on their SIMD, have two of each.  Per output cell the
// accumulator sees the same MFMAs in the same order and the epilogue the same steps, so the bits are the same.  The fused
// job is progressive where the late half was (the hazard rule is the stage's, add_stage).  `list`, `index`: where a job
// comes from (a fused one: p's half).  false: the two lists do not have pg.n_stages stages each.
struct SoloJob { NetJob job; int list, index; };
bool solo_halves_pair(const NetJob& a, const NetJob& b) {
  return ((a.og == 5 && b.og == 6) || (a.og == 6 && b.og == 5)) && a.w_off == b.w_off && a.wx_off == b.wx_off &&
         a.kgroups == b.kgroups && a.src == b.src && a.dst == b.dst && a.dtile == b.dtile && a.res == b.res &&
         a.act == b.act && a.extra == b.extra && a.sslot == b.sslot && a.nt == b.nt &&
         a.dst >= 0 && a.dst < NET_ACT_BUFFERS && a.sslot != NET_SSLOT_SPLIT;
}
bool solo_list(const NetProgram& pg, int p, bool whole_tile, std::vector<SoloJob>& out, int32_t& first_w) {
  const int lists[2] = {p, p ^ (NET_WAVES_HOST / 2)};
  int at[2] = {0, 0};
  out.clear();
  for (int s = 0; s < pg.n_stages; ++s) {
    const size_t begin = out.size();
    for (int k = 0; k < 2; ++k) {
      bool ended = false;
      while (!ended && at[k] < pg.n_jobs[lists[k]]) {
        out.push_back({pg.jobs[lists[k]][at[k]], lists[k], at[k]});
        ended = (out.back().job.flags & NET_JOB_STAGE_END) != 0;
        ++at[k];
      }
      if (!ended) return false;
      if (k == 0) out.back().job.flags &= ~NET_JOB_STAGE_END;     // the barrier comes after the other list's jobs
    }
    if (whole_tile && out.size() == begin + 2 && solo_halves_pair(out[begin].job, out[begin + 1].job)) {
      NetJob& j = out[begin].job;
      j.og = 0;
      j.flags = (int8_t)(NET_JOB_STAGE_END | ((j.flags | out[begin + 1].job.flags) & NET_JOB_PROGRESSIVE));
      out.pop_back();
    }
  }
  if (at[0] != pg.n_jobs[lists[0]] || at[1] != pg.n_jobs[lists[1]]) return false;
  int32_t next = -1;
  for (size_t i = out.size(); i-- > 0;) {        // prefetch chain, as for the waves' own lists
    out[i].job.next_w_off = next;
    if (out[i].job.og != OG_NONE && out[i].job.kgroups > 0) next = out[i].job.w_off;
  }
  first_w = next;
  return true;
}

// What nz_engine_set_weights derives from the description alone: no device, no weight values.
struct ConvShape { int cout, cin, k; };
struct NetLayout {
  bool recall;
  int iterations, trunk_tensors, trunk_k;
  std::vector<ConvShape> shapes;                 // in state_dict order
  int cin_main(int i, int in_planes) const {     // channels read from an activation buffer; the rest are the input planes
    const bool with_planes = (i == 0) || (recall && i == 1);
    return with_planes ? shapes[i].cin - in_planes : shapes[i].cin;
  }
};
std::string text(const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return buf;
}
// "" or what is wrong with the description
std::string net_layout(const nz_net_desc* net, int recurrent_iterations, NetLayout& L) {
  if (net->hex) return "hexagonal convolutions are built for nz_boardnet_* only";
  if (net->in_channels != 2 || net->policy_channels != 1) return "Tic-Tac-Toe nets take 2 input planes and 1 policy plane";
  if (net->width <= 0 || net->width > 64 || net->width % 4 != 0) return "width must be a multiple of 4 in (0, 64]";
  if (net->num_blocks < 0 || recurrent_iterations < 0) return "negative block/iteration count";
  const int arch = net->arch;
  if (arch != NZ_ARCH_RECURRENT && arch != NZ_ARCH_RESNET && arch != NZ_ARCH_CONVNET) return text("unknown architecture %d", arch);
  L.trunk_k = arch == NZ_ARCH_CONVNET ? net->kernel_size : 3;
  if (L.trunk_k != 1 && L.trunk_k != 3) return "ConvNet kernel_size must be 1 or 3";
  L.recall = arch == NZ_ARCH_RECURRENT && net->recall;
  L.iterations = arch == NZ_ARCH_RECURRENT ? recurrent_iterations : 1;
  L.trunk_tensors = arch == NZ_ARCH_CONVNET ? 1 + net->num_blocks : 1 + (L.recall ? 1 : 0) + 2 * net->num_blocks;
  if (1 + L.iterations * (L.trunk_tensors - 1) + 24 > NET_MAX_JOBS)
    return text("too many layers for one fused launch (%d iterations)", recurrent_iterations);
  const int W = net->width, IN = net->in_channels;
  std::vector<ConvShape>& shapes = L.shapes;
  shapes.clear();
  shapes.push_back({W, IN, L.trunk_k});
  if (L.recall) shapes.push_back({W, W + IN, 3});
  for (int i = (int)shapes.size(); i < L.trunk_tensors; ++i) shapes.push_back({W, W, L.trunk_k});
  const std::vector<int> pc = head_channels(W, net->policy_channels, 2), vc = head_channels(W, 1, 4);
  for (int i = 0; i < 2; ++i) shapes.push_back({pc[i + 1], pc[i], 3});
  for (int i = 0; i < 4; ++i) shapes.push_back({vc[i + 1], vc[i], 3});
  return "";
}
// The trunk's stages, one conv each, in execution order: activation areas 0 / 1 ping-pong from `cur` = 0, and on return
// `cur` holds the trunk's output.  The one layer list of both compilers (compile_net, compile_net_packed).
std::vector<StageConv> trunk_stages(const nz_net_desc* net, const NetLayout& L, int& cur) {
  std::vector<StageConv> out;
  cur = 0;
  if (net->arch == NZ_ARCH_CONVNET) {                                 // ConvNet.py:20-40: (conv, ELU) x (1 + num_layers)
    out.push_back({0, 0, cur, -1, 3, true});
    for (int i = 1; i < L.trunk_tensors; ++i) { out.push_back({i, cur, cur ^ 1, -1, 3, true}); cur ^= 1; }
  } else {
    out.push_back({0, 0, cur, -1, 1, true});                          // projection / input block + ReLU
    const int first_block = L.recall ? 2 : 1;
    for (int it = 0; it < L.iterations; ++it) {
      if (L.recall) { out.push_back({1, cur, cur ^ 1, -1, 0, true}); cur ^= 1; }    // cat([thought, x]) conv, no activation
      for (int b = 0; b < net->num_blocks; ++b) {                         // relu(conv2(relu(conv1(t))) + t)
        out.push_back({first_block + 2 * b, cur, cur ^ 1, -1, 1, true});
        out.push_back({first_block + 2 * b + 1, cur ^ 1, cur, cur, 1, true});
      }
    }
  }
  return out;
}

// The packed pass's program for P positions (net_packed_dev.hpp): the same layer list and weight offsets as compile_net,
// jobs of (conv, output tile, run of column tiles).  Areas 0 / 1 ping-pong through the trunk; the heads run side by
// side in four stages as in compile_net, the policy head's first conv into area 2 (no strip).  `tensor_of[w][j]`
// (optional): the conv tensor of pg.jobs[w][j], -1 for a barrier-only job.  "" or why it does not fit.
std::string compile_net_packed(const nz_net_desc* net, const NetLayout& L, const std::vector<PackedConv>& convs, int P,
                               NetProgram& pg, std::vector<int>* tensor_of = nullptr) {
  if (P < 1 || P > NET_PACKED_MAX) return text("positions per pass must be 1 .. %d", NET_PACKED_MAX);
  memset(&pg, 0, sizeof(pg));
  const int T = net_packed_tiles(P);
  bool ok = true;
  auto stage = [&](const std::vector<StageConv>& cs) {
    struct Unit { NetJob job; int cost, tensor; };
    int n_tiles = 0;
    for (const StageConv& sc : cs) n_tiles += convs[sc.tensor].ntiles;
    // runs as long as NET_PACKED_RUN allows while every wave still gets a unit, else shorter ones
    int run = NET_PACKED_RUN;
    while (run > 1 && n_tiles * ((T + run - 1) / run) < NET_WAVES_HOST) --run;
    const int n_runs = (T + run - 1) / run;
    std::vector<Unit> units;
    for (const StageConv& sc : cs) {
      const PackedConv& pc = convs[sc.tensor];
      for (int nt = 0; nt < pc.ntiles; ++nt)
        for (int r = 0, t0 = 0; r < n_runs; ++r) {
          const int len = T / n_runs + (r < T % n_runs ? 1 : 0);      // as even as T allows, longer runs first
          NetJob j{};
          j.w_off = pc.w_off + nt * pc.kgroups * NET_KG_DWORDS;
          j.wx_off = pc.wx_off + nt * 9 * 64;
          j.kgroups = (int8_t)pc.kgroups;
          j.nt = (int16_t)nt;
          j.extra = (int8_t)pc.extra;
          j.og = (int8_t)net_packed_og(t0, len);
          j.src = (int8_t)sc.src; j.dst = (int8_t)sc.dst; j.res = (int8_t)sc.res; j.act = (int8_t)sc.act;
          j.dtile = (int8_t)nt;
          units.push_back({j, len * 9 * (3 * pc.kgroups + pc.extra) + JOB_OVERHEAD, sc.tensor});
          t0 += len;
        }
    }
    std::stable_sort(units.begin(), units.end(), [](const Unit& a, const Unit& b) { return a.cost > b.cost; });
    int load[NET_WAVES_HOST] = {}, first[NET_WAVES_HOST];
    for (int w = 0; w < NET_WAVES_HOST; ++w) first[w] = pg.n_jobs[w];
    auto push = [&](int w, const NetJob& j, int tensor) {
      if (pg.n_jobs[w] >= NET_MAX_JOBS) { ok = false; return; }
      pg.jobs[w][pg.n_jobs[w]++] = j;
      if (tensor_of) tensor_of[w].push_back(tensor);
    };
    for (const Unit& u : units) {
      int w = 0;
      for (int i = 1; i < NET_WAVES_HOST; ++i)
        if (load[i] < load[w]) w = i;
      load[w] += u.cost;
      push(w, u.job, u.tensor);
    }
    for (int w = 0; w < NET_WAVES_HOST && ok; ++w) {
      if (pg.n_jobs[w] == first[w]) {            // nothing to do in this stage: barrier only
        NetJob j{};
        j.og = OG_NONE;
        push(w, j, -1);
      }
      if (ok) pg.jobs[w][pg.n_jobs[w] - 1].flags |= NET_JOB_STAGE_END;
    }
    ++pg.n_stages;
  };
  int cur = 0;
  for (const StageConv& sc : trunk_stages(net, L, cur)) stage({sc});
  const int ph = L.trunk_tensors, vh = ph + 2;
  const int vact = net->value_activation == NZ_ACT_RELU ? 1 : 2;
  const int side = cur ^ 1, pol = 2;
  stage({{vh, cur, side, -1, vact, true}, {ph, cur, pol, -1, 1, true}});
  stage({{vh + 1, side, cur, -1, vact, true}, {ph + 1, pol, NET_PACKED_DST_POLICY, -1, 0, true}});
  stage({{vh + 2, cur, side, -1, vact, true}});
  stage({{vh + 3, side, NET_PACKED_DST_VALUE, -1, 0, true}});
  if (!ok) return text("network too deep for one fused launch (%d iterations)", L.iterations);
  for (int w = 0; w < NET_WAVES_HOST; ++w) {     // prefetch chain, as in compile_net
    int32_t next = -1;
    for (int j = pg.n_jobs[w] - 1; j >= 0; --j) {
      pg.jobs[w][j].next_w_off = next;
      if (pg.jobs[w][j].og != OG_NONE && pg.jobs[w][j].kgroups > 0) next = pg.jobs[w][j].w_off;
    }
    pg.first_w_off[w] = next;
  }
  return "";
}

// The network as per-wave job lists (`convs`: the packed tensors' layout); `flops`: in-bounds taps only, 2 * Cout * Cin *
// 49 per 3x3 conv application (9 for 1x1).  "" or why it does not fit one fused launch.
std::string compile_net(const nz_net_desc* net, const NetLayout& L, const std::vector<PackedConv>& convs, NetProgram& pg,
                        double& flops, std::vector<int>* tensor_of = nullptr) {
  const std::vector<ConvShape>& shapes = L.shapes;
  const int trunk_tensors = L.trunk_tensors, iterations = L.iterations;
  flops = 0.0;
  // stages; activation buffers 0/1 ping-pong, `cur` holds the running trunk output.
  // act: 1 relu, 2 tanh, 3 elu
  memset(&pg, 0, sizeof(pg));
  bool ok = true;
  int cur = 0;
  auto stage = [&](std::vector<StageConv> convs_in_stage) {
    for (const StageConv& sc : convs_in_stage)
      flops += 2.0 * shapes[sc.tensor].cout * shapes[sc.tensor].cin * (shapes[sc.tensor].k == 3 ? 49.0 : 9.0);
    ok = ok && add_stage(pg, convs, convs_in_stage, tensor_of);
  };
  for (const StageConv& sc : trunk_stages(net, L, cur)) stage({sc});
  const int ph = trunk_tensors, vh = ph + 2;
  const int vact = net->value_activation == NZ_ACT_RELU ? 1 : 2;
  const int side = cur ^ 1;
  // The two heads side by side, four stages: both first convs read the trunk output, the value head's into `side`'s
  // first tiles, the policy head's into the tiles after them and past the fourth into the strip (64 channels: 48 + 32
  // = 3 + 2 tiles); then both second convs (the trunk output is dead: the value head's goes there), then the value
  // head's last two.  The policy head's second conv reads its K group from where the first wrote it: slots 2 tv0.. of
  // `side`, or slots 6-7 and the strip.
  const int tv0 = convs[vh].ntiles, tp0 = convs[ph].ntiles;
  if (tv0 + tp0 > 5 || (tv0 + tp0 == 5 && tv0 != 3)) return text("head layout: %d + %d tiles", tv0, tp0);
  const int p1_sslot = tv0 + tp0 <= 4 ? 2 * tv0 : NET_SSLOT_SPLIT;
  stage({{vh, cur, side, -1, vact, true, 0, 0}, {ph, cur, side, -1, 1, true, 0, tv0}});
  stage({{vh + 1, side, cur, -1, vact, true}, {ph + 1, side, NET_DST_POLICY, -1, 0, true, p1_sslot, 0}});
  stage({{vh + 2, cur, side, -1, vact, true}});
  stage({{vh + 3, side, NET_DST_VALUE, -1, 0, true}});                      // per-cell outputs; net_tile takes the mean
  if (!ok) return text("network too deep for one fused launch (%d iterations)", iterations);
  for (int w = 0; w < NET_WAVES_HOST; ++w) {     // prefetch chain: each job names the next weight stream
    int32_t next = -1;
    for (int j = pg.n_jobs[w] - 1; j >= 0; --j) {
      pg.jobs[w][j].next_w_off = next;
      if (pg.jobs[w][j].og != OG_NONE && pg.jobs[w][j].kgroups > 0) next = pg.jobs[w][j].w_off;
    }
    pg.first_w_off[w] = next;
  }
  // Simulations a row of a wave that sits the pass out may run under each stage (selfplay.hip burst_under_pass), from
  // the stage's length in add_stage's cost model: a four-tile stage of two K groups (26 x 6 + 12 = 168 units on its
  // longest wave) covers two, anything shorter one.
  {
    int budget[2] = {2, 1};
    if (const char* v = getenv("NZ_BURST_BUDGET")) {          // tuning experiments: "long,short"
      int a = 0, b = 0;
      if (sscanf(v, "%d,%d", &a, &b) == 2) { budget[0] = std::max(0, a); budget[1] = std::max(0, b); }
    }
    for (int s = 0; s < pg.n_stages; ++s) pg.stage_budget[s] = budget[pg.stage_budget[s] >= BURST_LONG_STAGE ? 0 : 1];
  }
  // The lists of a stealing pass (NetProgram::solo_jobs).  NZ_BURST_WHOLE_TILE=0 (tuning experiments): the pure
  // concatenation, two half-tile jobs where one whole-tile job would do.
  bool whole_tile = true;
  if (const char* v = getenv("NZ_BURST_WHOLE_TILE")) whole_tile = atoi(v) != 0;
  for (int p = 0; p < NET_WAVES_HOST; ++p) {
    std::vector<SoloJob> solo;
    if (!solo_list(pg, p, whole_tile, solo, pg.solo_first_w[p]) || solo.size() > (size_t)NET_MAX_SOLO_JOBS)
      return "job lists disagree on the number of stages";
    int stage_ends = 0;
    for (size_t i = 0; i < solo.size(); ++i) {
      pg.solo_jobs[p][i] = solo[i].job;
      stage_ends += (solo[i].job.flags & NET_JOB_STAGE_END) ? 1 : 0;
    }
    // (the sitting-out wave counts the barriers off its own list: selfplay.hip burst_under_pass)
    if (stage_ends != pg.n_stages) return "job lists disagree on the number of stages";
    pg.solo_n_jobs[p] = (int32_t)solo.size();
  }
  return "";
}

// The engine's packed program for P positions per pass, on the device: compiled for the current weights at first use.
nz_status packed_program(nz_engine* e, int P, const NetProgram** out) {
  if (P < 1 || P > NET_PACKED_MAX) return fail(e, NZ_ERR_ARG, "positions per pass must be 1 .. %d", NET_PACKED_MAX);
  if (!e->packed_ready[P]) {
    NetLayout L;
    std::string bad = net_layout(&e->net, e->iters, L);
    std::unique_ptr<NetProgram> pg(new NetProgram);
    if (bad.empty()) bad = compile_net_packed(&e->net, L, e->convs, P, *pg);
    if (!bad.empty()) return fail(e, NZ_ERR_ARG, "%s", bad.c_str());
    if (!e->packed_prog[P].ensure(1)) return fail(e, NZ_ERR_HIP, "device allocation failed (packed program)");
    NZ_HIP(e, hipMemcpy(e->packed_prog[P].get(), pg.get(), sizeof(NetProgram), hipMemcpyHostToDevice));
    e->packed_ready[P] = true;
  }
  *out = e->packed_prog[P].get();
  return NZ_OK;
}

// the layout compile_net and compile_net_packed need when no weights are at hand (host-only queries): zero weights
std::string layout_only(const nz_net_desc* net, int recurrent_iterations, NetLayout& L, std::vector<PackedConv>& convs) {
  const std::string bad = net_layout(net, recurrent_iterations, L);
  if (!bad.empty()) return bad;
  std::vector<float> packed;
  convs.resize(L.shapes.size());
  for (size_t i = 0; i < L.shapes.size(); ++i) {
    const std::vector<float> zeros((size_t)L.shapes[i].cout * L.shapes[i].cin * 9, 0.f);
    convs[i] = pack_conv(zeros.data(), L.shapes[i].cout, L.shapes[i].cin, L.cin_main((int)i, net->in_channels), packed);
  }
  return "";
}

hipStream_t as_stream(void* s) { return static_cast<hipStream_t>(s); }

nz_status check_device_flag(nz_engine* e, hipStream_t s) {
  int32_t flag = 0;
  NZ_HIP(e, hipMemcpyAsync(&flag, e->tp.error_flag, sizeof(flag), hipMemcpyDeviceToHost, s));
  NZ_HIP(e, hipStreamSynchronize(s));
  if (flag != 0)
    return fail(e, NZ_ERR_OVERFLOW, "device check failed (flag %d: 1 = tree arena full, 2 = visit table too short, "
                                    "4 = move finished before its search, 8 = forced action is not legal, "
                                    "64 = persistent kernel gave up after its cycle bound)", flag);
  return NZ_OK;
}

// ---- start positions (nz_engine_reset_to, nz_engine_match_play_from, nz_engine_policy_actions) ------------------------
// The one check of a position a caller names: nullptr when it is playable, else the condition it
// fails.  How the position arose is not checked.
const char* ttt_unplayable(uint32_t b) {
  auto line = [](uint32_t m) {
    return (m & 0007u) == 0007u || (m & 0070u) == 0070u || (m & 0700u) == 0700u || (m & 0111u) == 0111u ||
           (m & 0222u) == 0222u || (m & 0444u) == 0444u || (m & 0421u) == 0421u || (m & 0124u) == 0124u;
  };
  if (b & ~0x01ff01ffu) return "a bit outside the stone sets (bits 0-8 and 16-24) is set";
  const uint32_t p1 = b & 0x1ffu, p2 = (b >> 16) & 0x1ffu;
  if (p1 & p2) return "a cell holds a stone of both players";
  const int diff = __builtin_popcount(p1) - __builtin_popcount(p2);
  if (diff != 0 && diff != 1) return "stones(p1) - stones(p2) is neither 0 nor 1";
  if (line(p1) || line(p2)) return "a side has a line: the game is over";
  if ((p1 | p2) == 0x1ffu) return "no cell is empty";
  return nullptr;
}
// what the kernels of ttt_agents.hip borrow of the first n matches' state
TttMatchArgs match_args(MatchArrays& m, int n) {
  TttMatchArgs a{};
  a.n = n;
  a.board = m.board.get(); a.alive = m.alive.get(); a.length = m.length.get(); a.outcome = m.outcome.get();
  a.actions = m.actions.get(); a.forced = m.forced.get(); a.err = m.err.get();
  a.states = m.states.get(); a.probs = m.probs.get();
  for (int i = 0; i < 2; ++i) {
    a.agent_actions[i] = m.agent_actions[i].get(); a.agent_n_legal[i] = m.agent_n_legal[i].get();
    a.mt_keys[i] = m.mt_keys[i].get(); a.mt_pos[i] = m.mt_pos[i].get();
  }
  return a;
}
// Every board playable, and with `same_ply` all at one stone count (returned in *stones); else the refusal's words.
bool check_start_boards(const uint32_t* boards, int n, bool same_ply, int* stones, std::string& msg) {
  for (int i = 0; i < n; ++i) {
    const char* why = ttt_unplayable(boards[i]);
    if (why) {
      msg = text("start board %d (0x%08x) is not playable: %s", i, boards[i], why);
      return false;
    }
  }
  const int k0 = __builtin_popcount(boards[0]);
  for (int i = 1; same_ply && i < n; ++i) {
    const int k = __builtin_popcount(boards[i]);
    if (k != k0) {
      msg = text("start boards 0 and %d hold %d and %d stones: every match of a round starts at the same ply", i, k0, k);
      return false;
    }
  }
  if (stones) *stones = k0;
  return true;
}

}  // namespace

extern "C" {

const char* nz_version(void) { return "nuzero_amd 0.1 (gfx950)"; }

const char* nz_last_error(const nz_engine* e) { return e ? e->error.c_str() : g_create_error.c_str(); }

nz_status nz_engine_create(nz_engine** out, const nz_search_cfg* cfg, const nz_game_desc* game, int32_t n_games,
                           int32_t device) {
  return nz_engine_create_ex(out, cfg, game, n_games, n_games, device);
}

nz_status nz_engine_create_ex(nz_engine** out, const nz_search_cfg* cfg, const nz_game_desc* game, int32_t n_slots,
                              int32_t n_games, int32_t device) {
  if (!out || !cfg || !game) return fail(nullptr, NZ_ERR_ARG, "null argument");
  if (n_slots <= 0) return fail(nullptr, NZ_ERR_ARG, "n_slots must be positive");
  if (n_slots > n_games) n_slots = n_games > 0 ? n_games : n_slots;
  *out = nullptr;
  if (game->game != NZ_GAME_TIC_TAC_TOE) return fail(nullptr, NZ_ERR_ARG, "unsupported game %d", game->game);
  if (n_games <= 0) return fail(nullptr, NZ_ERR_ARG, "n_games must be positive");
  if (cfg->mcts_simulations <= 0) return fail(nullptr, NZ_ERR_ARG, "mcts_simulations must be positive");
  if (!cfg->keep_subtree)
    return fail(nullptr, NZ_ERR_ARG, "keep_subtree = False is not supported: the reference never resets the root "
                                     "in that mode (Training/Gamer.py:78-79) and every shipped config sets True");
  if (!(cfg->pb_c_base > 0)) return fail(nullptr, NZ_ERR_ARG, "pb_c_base must be positive");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
    return fail(nullptr, NZ_ERR_HIP, "no HIP device available (the engine has no CPU fallback)");
  if (device < 0 || device >= n_dev) return fail(nullptr, NZ_ERR_ARG, "device %d out of range", device);

  nz_engine* e = new nz_engine;
  e->cfg = *cfg;
  e->game = *game;
  e->device = device;
  e->n_games = n_games;
  e->n_slots = n_slots;
  // every expansion at move m adds at most 9 - m children: 1 + sims * (9 + 8 + ... + 1)
  e->cap = 1 + cfg->mcts_simulations * 45;
  e->tab_len = cfg->mcts_simulations * TTT_MAX_MOVES + 2;
  auto bail = [&](nz_status s) {
    g_create_error = e->error;
    nz_engine_destroy(e);
    return s;
  };
  if (hipSetDevice(device) != hipSuccess) return bail(fail(e, NZ_ERR_HIP, "hipSetDevice(%d) failed", device));

  TreeParams& p = e->tp;
  memset(&p, 0, sizeof(p));
  const size_t G = n_games, N = (size_t)n_slots * (size_t)e->cap, GT = G * TTT_MAX_MOVES, GTA = GT * TTT_ACTIONS;
#define P(f, n)                                                                           \
  if (!e->dev.f.ensure(n)) return bail(fail(e, NZ_ERR_HIP, "device allocation failed")); \
  p.f = e->dev.f.get()
  P(nodes, N);
  P(board, G); P(length, G); P(alive, G); P(outcome, G); P(root, G); P(node_count, G);
  P(sims_left, G); P(pending, G); P(leaf_board, G); P(path, G * MAX_PATH); P(path_len, G);
  P(sim_count, G); P(exp_count, G); P(sel_nodes, G); P(sel_children, G); P(new_nodes, G); P(desync, G); P(n_root_children, G);
  P(leaf_count, 2); P(leaf_boards, G); P(leaf_logits, G * TTT_ACTIONS); P(leaf_value, G);
  P(error_flag, 1);
  P(hist_board, GT); P(hist_action, GT); P(hist_visits, GTA); P(hist_tree_size, GT);
  P(hist_children, GT); P(hist_bias, GT); P(hist_prior, GTA); P(hist_value_sum, GTA);
  P(hist_root_value_sum, GT);
  P(bias_tab, e->tab_len); P(sqrt_tab, e->tab_len);
  P(next_game, 1);
#undef P
  EngineArrays& d = e->dev;
  if (!d.noise.ensure(G * TTT_ACTIONS) || !d.uniforms.ensure(G * 3) || !d.game_noise.ensure(GTA) ||
      !d.game_uniforms.ensure(GT * 3) || !d.stamps.ensure((size_t)n_slots * 8) ||      // (one workgroup per slot at most)
      !d.prog.ensure(1))
    return bail(fail(e, NZ_ERR_HIP, "device allocation failed"));
  p.cap = e->cap;
  p.n_games = n_games;
  p.n_slots = n_slots;
  p.table = nullptr;
  p.tab_len = e->tab_len;
  p.sims = cfg->mcts_simulations;
  p.negate_player = game->negate_player;
  p.value_factor = cfg->value_factor;
  p.frac = cfg->root_exploration_fraction;
  p.one_minus_frac = 1.0 - cfg->root_exploration_fraction;
  p.training = cfg->training;
  p.softmax_moves = cfg->number_of_softmax_moves;
  p.eps_softmax = cfg->epsilon_softmax_exploration;
  p.eps_random = cfg->epsilon_random_exploration;
  {   // a workgroup's 16 network rows are filled only when there are 16 slots for every CU: fewer slots are spread over the
      // chip (1024 slots: 4 to each of 256 workgroups instead of 16 to each of 64 -- a pass costs the same matrix
      // instructions however many of its columns hold a leaf, and a tree phase waits for the slowest of fewer rows)
    hipDeviceProp_t prop;
    int n_cu = 256;
    if (hipGetDeviceProperties(&prop, e->device) == hipSuccess && prop.multiProcessorCount > 0) n_cu = prop.multiProcessorCount;
    p.slots_per_wg = std::min(16, std::max(1, (n_slots + n_cu - 1) / n_cu));
    if (const char* v = getenv("NZ_SLOTS_PER_WG")) p.slots_per_wg = std::min(16, std::max(1, atoi(v)));   // tuning experiments
  }
  // a row runs at most this many simulations between two network passes (results do not depend on it).  With four slots to
  // a workgroup more helps at 100 simulations a move (1024 slots, one box: 6 / 10 / 16 / 32 -> 28.8 / 30.1 / 30.8 / 31.4 k
  // games/s) and hurts at configs[2]'s 400 (12 / 16 / 24 / 32 -> 8.76 / 8.68 / 8.52 / 8.52 k): 16 everywhere
  p.sims_per_cycle = 16;
  // A wave whose row hit that cap sits out the network pass and goes on simulating under it, while the other wave of its
  // SIMD runs both waves' jobs (selfplay.hip burst_under_pass; results do not depend on it).  A capped row then no longer
  // holds the tree phase for all its simulations, so full workgroups take a lower cap: 4096 slots, one box, switch on,
  // cap 4 / 6 / 8 / 12 / 16 -> 122.7 / 124.3 / 123.7 / 121.8 / 121.3 k games/s beside 120.6-121.0 k without the switch
  // (profiles/r06_burst_under_net.txt).
  p.burst_under_net = 1;
  if (const char* v = getenv("NZ_BURST_UNDER_NET")) p.burst_under_net = std::min(2, std::max(0, atoi(v)));   // tuning experiments
  // An engine of at most NET_PACKED_DEFAULT games per workgroup takes the packed pass (net_packed_dev.hpp; the same
  // outputs, fewer matrix instructions).  NZ_NET_PACKED (experiments): 0 = never, N = for slots_per_wg <= N.  The packed
  // pass has no stealing partner, so for such an engine burst_under_net counts as off (results do not depend on it).
  {
    int upto = NET_PACKED_DEFAULT;
    if (const char* v = getenv("NZ_NET_PACKED")) upto = std::min(NET_PACKED_MAX, std::max(0, atoi(v)));
    e->packed = p.slots_per_wg <= upto;
    if (e->packed) p.burst_under_net = 0;
  }
  if (p.burst_under_net == 1 && p.slots_per_wg == 16) p.sims_per_cycle = 6;
  if (const char* v = getenv("NZ_SIMS_PER_CYCLE")) p.sims_per_cycle = std::max(1, atoi(v));   // tuning experiments
  e->f32_packed = e->packed;
  e->f32_burst = p.burst_under_net;
  e->f32_sims_per_cycle = p.sims_per_cycle;
  {   // every cycle finishes at least one simulation or one move of every live row of the workgroup
    const double games_per_slot = std::ceil((double)p.n_games / (double)p.n_slots) + 2.0;
    const double bound = 16.0 * games_per_slot * TTT_MAX_MOVES * ((double)cfg->mcts_simulations + 2.0);
    p.max_cycles = (int32_t)std::min(bound, 2.0e9);
  }

  // Explorer.calculate_exploration_bias / calculate_ucb_factor (Explorer.py:103-112):
  // log() and sqrt() of the parent visit count, from the host libm
  std::vector<double> hb(e->tab_len), hs(e->tab_len);
  for (int n = 0; n < e->tab_len; ++n) {
    hb[n] = std::log(((double)n + cfg->pb_c_base + 1.0) / cfg->pb_c_base) + cfg->pb_c_init;
    hs[n] = std::sqrt((double)n);
  }
  if (hipMemcpy(d.bias_tab.get(), hb.data(), hb.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d.sqrt_tab.get(), hs.data(), hs.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    return bail(fail(e, NZ_ERR_HIP, "table upload failed"));

  if (!e->h_children.ensure(G) || !e->h_alive.ensure(G) || !e->h_noise.ensure(G * TTT_ACTIONS) || !e->h_uniforms.ensure(G * 3) ||
      !e->h_game_noise.ensure(GTA) || !e->h_game_uniforms.ensure(GT * 3) || !e->h_next_noise.ensure(GTA) ||
      !e->h_next_uniforms.ensure(GT * 3) || !e->h_desync.ensure(G))
    return bail(fail(e, NZ_ERR_HIP, "pinned host allocation failed"));
  for (PinnedBuf<double>* b : {&e->h_noise, &e->h_uniforms, &e->h_game_noise, &e->h_game_uniforms, &e->h_next_noise, &e->h_next_uniforms})
    memset(b->get(), 0, b->size() * sizeof(double));

  launch_reset(p, nullptr, nullptr);
  if (hipDeviceSynchronize() != hipSuccess) return bail(fail(e, NZ_ERR_HIP, "reset kernel failed"));
  *out = e;
  return NZ_OK;
}

void nz_engine_destroy(nz_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  (void)hipDeviceSynchronize();
  if (e->fallback) nz_engine_destroy(e->fallback);
  for (nz_rng* r : e->rngs) nz_rng_destroy(r);
  delete e;
}

nz_status nz_engine_dims(const nz_engine* e, nz_dims* out) {
  if (!e || !out) return NZ_ERR_ARG;
  out->n_games = e->n_games;
  out->n_slots = e->n_slots;
  out->num_actions = TTT_ACTIONS;
  out->max_moves = TTT_MAX_MOVES;
  out->state_channels = 2;
  out->rows = 3;
  out->cols = 3;
  out->node_capacity = e->cap;
  return NZ_OK;
}

nz_status nz_engine_set_weights(nz_engine* e, const nz_net_desc* net, const float* const* weights,
                                int32_t n_tensors, int32_t recurrent_iterations) {
  if (!e || !net || !weights) return NZ_ERR_ARG;
  NetLayout L;
  const std::string bad = net_layout(net, recurrent_iterations, L);
  if (!bad.empty()) return fail(e, NZ_ERR_ARG, "%s", bad.c_str());
  const int expect = (int)L.shapes.size();
  if (n_tensors != expect) return fail(e, NZ_ERR_ARG, "expected %d weight tensors, got %d", expect, n_tensors);
  NZ_HIP(e, hipSetDevice(e->device));
  const std::vector<ConvShape>& shapes = L.shapes;

  std::vector<std::vector<float>> host(n_tensors);
  for (int i = 0; i < n_tensors; ++i) {
    const size_t n_in = (size_t)shapes[i].cout * shapes[i].cin * shapes[i].k * shapes[i].k;
    std::vector<float> raw(n_in);
    NZ_HIP(e, hipMemcpy(raw.data(), weights[i], n_in * sizeof(float), hipMemcpyDefault));
    if (shapes[i].k == 3) {
      host[i].swap(raw);
    } else {                                   // 1x1 conv = a 3x3 conv whose only tap is the centre
      host[i].assign((size_t)shapes[i].cout * shapes[i].cin * 9, 0.f);
      for (size_t j = 0; j < n_in; ++j) host[i][j * 9 + 4] = raw[j];
    }
  }

  std::vector<float> packed;
  std::vector<PackedConv> convs(n_tensors);
  for (int i = 0; i < n_tensors; ++i) {
    convs[i] = pack_conv(host[i].data(), shapes[i].cout, shapes[i].cin, L.cin_main(i, net->in_channels), packed, e->prec);
  }

  NetProgram& pg = e->prog_host;
  double flops = 0.0;
  const std::string deep = compile_net(net, L, convs, pg, flops);
  if (!deep.empty()) return fail(e, NZ_ERR_ARG, "%s", deep.c_str());
  e->algorithmic_flops_per_position = flops;
  {   // what the matrix cores execute for one tile of 16 positions (net_dev.hpp): six bf16 MFMAs per
      // (input cell, tap) pair and 32-channel K group (plain-bf16 mode: one), one float32 MFMA per pair for the input planes
    const double terms = e->prec == NZ_PREC_BF16 ? 1.0 : 6.0;
    double bf16 = 0.0, f32 = 0.0;
    for (int w = 0; w < NET_WAVES_HOST; ++w)
      for (int j = 0; j < pg.n_jobs[w]; ++j) {
        const NetJob& job = pg.jobs[w][j];
        if (job.og == OG_NONE) continue;
        bf16 += (double)og_taps[job.og] * job.kgroups * terms * (2.0 * 16 * 16 * 32);
        f32 += (double)og_taps[job.og] * job.extra * (2.0 * 16 * 16 * 4);
      }
    e->executed_bf16_flops_per_position = bf16 / 16.0;
    e->executed_f32_flops_per_position = f32 / 16.0;
  }

  if (!e->weights_dev.ensure(packed.size())) return fail(e, NZ_ERR_HIP, "device allocation failed (%zu packed weights)", packed.size());
  NZ_HIP(e, hipMemcpy(e->weights_dev.get(), packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
  NZ_HIP(e, hipMemcpy(e->dev.prog.get(), &pg, sizeof(pg), hipMemcpyHostToDevice));
  e->net = *net;
  e->iters = recurrent_iterations;
  e->have_net = true;
  e->have_table = false;
  e->tp.table = nullptr;
  e->convs = convs;
  for (bool& ready : e->packed_ready) ready = false;
  if (e->packed) {                               // the program nz_engine_play's kernel will run
    const NetProgram* unused = nullptr;
    const nz_status st = packed_program(e, e->tp.slots_per_wg, &unused);
    if (st != NZ_OK) return st;
  }
  return NZ_OK;
}

nz_status nz_net_program(const nz_net_desc* net, int32_t recurrent_iterations, int32_t* jobs, int32_t max_jobs,
                         int32_t* n_jobs) {
  if (!net || !n_jobs || (!jobs && max_jobs > 0)) return NZ_ERR_ARG;
  NetLayout L;
  std::string bad = net_layout(net, recurrent_iterations, L);
  std::vector<float> packed;
  std::vector<PackedConv> convs(L.shapes.size());
  NetProgram* pg = new NetProgram;
  if (bad.empty()) {
    for (size_t i = 0; i < L.shapes.size(); ++i) {   // the layout only: zero weights
      const std::vector<float> zeros((size_t)L.shapes[i].cout * L.shapes[i].cin * 9, 0.f);
      convs[i] = pack_conv(zeros.data(), L.shapes[i].cout, L.shapes[i].cin, L.cin_main((int)i, net->in_channels), packed);
    }
    double flops = 0.0;
    bad = compile_net(net, L, convs, *pg, flops);
  }
  if (!bad.empty()) {
    delete pg;
    g_create_error = bad;
    return NZ_ERR_ARG;
  }
  int32_t n = 0;
  for (int w = 0; w < NET_WAVES_HOST; ++w) {
    int stage = 0;
    for (int j = 0; j < pg->n_jobs[w]; ++j) {
      const NetJob& job = pg->jobs[w][j];
      if (job.og != OG_NONE) {
        if (n < max_jobs) {
          const int32_t row[NZ_NET_JOB_FIELDS] = {w, stage, job.og, og_mask(job.og), job.kgroups, job.sslot, job.src, job.dst,
                                                  job.res, job.act, job.dtile, job.extra,
                                                  (job.flags & NET_JOB_PROGRESSIVE) ? 1 : 0};
          memcpy(jobs + (size_t)n * NZ_NET_JOB_FIELDS, row, sizeof(row));
        }
        ++n;
      }
      if (job.flags & NET_JOB_STAGE_END) ++stage;
    }
  }
  delete pg;
  *n_jobs = n;
  return NZ_OK;
}

nz_status nz_net_steal_order(const nz_net_desc* net, int32_t recurrent_iterations, int32_t wave, int32_t* rows,
                             int32_t max_rows, int32_t* n_rows, int32_t* first_w) {
  if (!net || !n_rows || !first_w || (!rows && max_rows > 0) || wave < 0 || wave >= NET_WAVES_HOST) return NZ_ERR_ARG;
  NetLayout L;
  std::string bad = net_layout(net, recurrent_iterations, L);
  std::vector<float> packed;
  std::vector<PackedConv> convs(L.shapes.size());
  std::unique_ptr<NetProgram> pg(new NetProgram);
  if (bad.empty()) {
    for (size_t i = 0; i < L.shapes.size(); ++i) {   // the layout only: zero weights
      const std::vector<float> zeros((size_t)L.shapes[i].cout * L.shapes[i].cin * 9, 0.f);
      convs[i] = pack_conv(zeros.data(), L.shapes[i].cout, L.shapes[i].cin, L.cin_main((int)i, net->in_channels), packed);
    }
    double flops = 0.0;
    bad = compile_net(net, L, convs, *pg, flops);
  }
  if (!bad.empty()) {
    g_create_error = bad;
    return NZ_ERR_ARG;
  }
  // the concatenated order: the solo list without whole-tile jobs, whatever NZ_BURST_WHOLE_TILE says
  std::vector<SoloJob> solo;
  int32_t first = -1;
  if (!solo_list(*pg, wave, false, solo, first)) {
    g_create_error = "job lists disagree on the number of stages";
    return NZ_ERR_ARG;
  }
  int32_t n = 0;
  int stage = 0;
  for (const SoloJob& sj : solo) {
    const NetJob& job = sj.job;
    const bool end = (pg->jobs[sj.list][sj.index].flags & NET_JOB_STAGE_END) != 0;     // of the job's own list
    if (n < max_rows) {
      const int32_t row[NZ_NET_STEAL_FIELDS] = {sj.list, sj.index, stage, job.og, job.kgroups, job.w_off, job.next_w_off,
                                                job.dst, job.dtile, end ? 1 : 0, pg->stage_budget[stage]};
      memcpy(rows + (size_t)n * NZ_NET_STEAL_FIELDS, row, sizeof(row));
    }
    ++n;
    if (job.flags & NET_JOB_STAGE_END) ++stage;
  }
  *n_rows = n;
  *first_w = first;
  return NZ_OK;
}

nz_status nz_net_solo_program(const nz_net_desc* net, int32_t recurrent_iterations, int32_t wave, int32_t* jobs,
                              int32_t max_jobs, int32_t* n_jobs, int32_t* first_w) {
  if (!net || !n_jobs || !first_w || (!jobs && max_jobs > 0) || wave < 0 || wave >= NET_WAVES_HOST) return NZ_ERR_ARG;
  NetLayout L;
  std::string bad = net_layout(net, recurrent_iterations, L);
  std::vector<float> packed;
  std::vector<PackedConv> convs(L.shapes.size());
  std::unique_ptr<NetProgram> pg(new NetProgram);
  if (bad.empty()) {
    for (size_t i = 0; i < L.shapes.size(); ++i) {   // the layout only: zero weights
      const std::vector<float> zeros((size_t)L.shapes[i].cout * L.shapes[i].cin * 9, 0.f);
      convs[i] = pack_conv(zeros.data(), L.shapes[i].cout, L.shapes[i].cin, L.cin_main((int)i, net->in_channels), packed);
    }
    double flops = 0.0;
    bad = compile_net(net, L, convs, *pg, flops);
  }
  if (!bad.empty()) {
    g_create_error = bad;
    return NZ_ERR_ARG;
  }
  // the very list net_tile walks: pg->solo_jobs[wave]; barrier-only jobs included
  int stage = 0;
  const int32_t n = pg->solo_n_jobs[wave];
  for (int32_t i = 0; i < n && i < max_jobs; ++i) {
    const NetJob& job = pg->solo_jobs[wave][i];
    const int end = (job.flags & NET_JOB_STAGE_END) ? 1 : 0;
    const int32_t row[NZ_NET_SOLO_FIELDS] = {wave, stage, job.og, og_mask(job.og), job.kgroups, job.sslot, job.src, job.dst,
                                             job.res, job.act, job.dtile, job.extra,
                                             (job.flags & NET_JOB_PROGRESSIVE) ? 1 : 0, job.w_off, job.next_w_off, end};
    memcpy(jobs + (size_t)i * NZ_NET_SOLO_FIELDS, row, sizeof(row));
    stage += end;
  }
  *n_jobs = n;
  *first_w = pg->solo_first_w[wave];
  return NZ_OK;
}

int32_t nz_net_final_tap(int32_t cell) { return cell >= 0 && cell < 9 ? net_final_tap(cell) : -1; }

nz_status nz_net_packed_columns(int32_t P, int32_t* col_pos, int32_t* col_cell, int32_t* tap_src, int32_t max_cols,
                                int32_t* n_tiles) {
  if (P < 1 || P > NET_PACKED_MAX || !col_pos || !col_cell || !tap_src || !n_tiles) return NZ_ERR_ARG;
  const int T = net_packed_tiles(P);
  if (16 * T > max_cols) return NZ_ERR_ARG;
  for (int i = 0; i < 16 * T; ++i) {             // column i % 16 of tile i / 16 holds pair i (net_packed_dev.hpp pk_column)
    const bool live = i < 9 * P;
    col_pos[i] = live ? i / 9 : -1;
    col_cell[i] = live ? i % 9 : -1;
    for (int tap = 0; tap < 9; ++tap) tap_src[9 * i + tap] = live ? net_packed_tap_source(i % 9, tap) : -1;
  }
  *n_tiles = T;
  return NZ_OK;
}

nz_status nz_net_packed_program(const nz_net_desc* net, int32_t recurrent_iterations, int32_t P, int32_t* jobs,
                                int32_t max_jobs, int32_t* n_jobs) {
  if (!net || !n_jobs || (!jobs && max_jobs > 0)) return NZ_ERR_ARG;
  NetLayout L;
  std::vector<PackedConv> convs;
  std::unique_ptr<NetProgram> pg(new NetProgram);
  std::vector<int> tensor_of[NET_WAVES_HOST];
  std::string bad = layout_only(net, recurrent_iterations, L, convs);
  if (bad.empty()) bad = compile_net_packed(net, L, convs, P, *pg, tensor_of);
  if (!bad.empty()) {
    g_create_error = bad;
    return NZ_ERR_ARG;
  }
  int32_t n = 0;
  for (int w = 0; w < NET_WAVES_HOST; ++w) {
    int stage = 0;
    for (int j = 0; j < pg->n_jobs[w]; ++j, ++n) {
      const NetJob& job = pg->jobs[w][j];
      const int tensor = tensor_of[w][j], end = (job.flags & NET_JOB_STAGE_END) ? 1 : 0;
      const bool work = job.og != OG_NONE;
      if (n < max_jobs) {
        const int32_t row[NZ_NET_PACKED_JOB_FIELDS] = {w, stage, tensor, job.nt, work ? job.og & 7 : 0, work ? job.og >> 3 : 0,
                                                       job.kgroups, job.src, job.dst, job.res, job.act, job.extra, end,
                                                       work ? convs[tensor].ntiles : 0};
        memcpy(jobs + (size_t)n * NZ_NET_PACKED_JOB_FIELDS, row, sizeof(row));
      }
      stage += end;
    }
  }
  *n_jobs = n;
  return NZ_OK;
}

nz_status nz_engine_positions_per_pass(const nz_engine* e, int32_t* out) {
  if (!e || !out) return NZ_ERR_ARG;
  *out = e->packed ? e->tp.slots_per_wg : 16;
  return NZ_OK;
}

nz_status nz_engine_set_table(nz_engine* e, const float* table, int32_t n_rows) {
  if (!e || !table) return NZ_ERR_ARG;
  if (n_rows != TTT_TABLE_ROWS) return fail(e, NZ_ERR_ARG, "table must have %d rows", TTT_TABLE_ROWS);
  NZ_HIP(e, hipSetDevice(e->device));
  if (!e->table_dev.ensure((size_t)TTT_TABLE_ROWS * 10)) return fail(e, NZ_ERR_HIP, "device allocation failed (table)");
  NZ_HIP(e, hipMemcpy(e->table_dev.get(), table, (size_t)TTT_TABLE_ROWS * 10 * sizeof(float), hipMemcpyDefault));
  e->tp.table = e->table_dev.get();
  e->have_table = true;
  return NZ_OK;
}

nz_status nz_engine_reset(nz_engine* e, void* stream) {
  if (!e) return NZ_ERR_ARG;
  NZ_HIP(e, hipSetDevice(e->device));
  Span sp(e, as_stream(stream), 2);
  launch_reset(e->tp, nullptr, as_stream(stream));
  NZ_HIP(e, hipGetLastError());
  return NZ_OK;
}

nz_status nz_engine_reset_to(nz_engine* e, const uint32_t* boards_host, void* stream) {
  if (!e || !boards_host) return fail(e, NZ_ERR_ARG, "nz_engine_reset_to: NULL %s", e ? "boards" : "engine");
  if (e->cfg.training)
    return fail(e, NZ_ERR_ARG, "a training engine starts every game at the empty board (start positions are for "
                               "evaluation engines: create it with training = 0)");
  if (e->n_slots != e->n_games)
    return fail(e, NZ_ERR_STATE, "start positions need the lock-step route: n_slots == n_games (every game of the round in flight)");
  std::string msg;
  if (!check_start_boards(boards_host, e->n_games, false, nullptr, msg)) return fail(e, NZ_ERR_ARG, "%s", msg.c_str());
  NZ_HIP(e, hipSetDevice(e->device));
  if (!e->dev.start_board.ensure((size_t)e->n_games)) return fail(e, NZ_ERR_HIP, "device allocation failed (start boards)");
  hipStream_t s = as_stream(stream);
  NZ_HIP(e, hipMemcpyAsync(e->dev.start_board.get(), boards_host, (size_t)e->n_games * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  Span sp(e, s, 2);
  launch_reset(e->tp, e->dev.start_board.get(), s);
  NZ_HIP(e, hipGetLastError());
  return NZ_OK;
}

nz_status nz_engine_root_children(nz_engine* e, int32_t* n_children_dev, void* stream) {
  if (!e || !n_children_dev) return NZ_ERR_ARG;
  NZ_HIP(e, hipMemcpyAsync(n_children_dev, e->tp.n_root_children, e->n_games * sizeof(int32_t),
                           hipMemcpyDeviceToDevice, as_stream(stream)));
  return NZ_OK;
}

nz_status nz_engine_alive(nz_engine* e, int32_t* alive_dev, void* stream) {
  if (!e || !alive_dev) return NZ_ERR_ARG;
  NZ_HIP(e, hipMemcpyAsync(alive_dev, e->tp.alive, e->n_games * sizeof(int32_t), hipMemcpyDeviceToDevice,
                           as_stream(stream)));
  return NZ_OK;
}

// noise + simulations of one move for every live game (no action yet)
static nz_status search_lockstep(nz_engine* e, const double* noise_dev, hipStream_t s) {
  const TreeParams& p = e->tp;
  if (e->cfg.training) {
    Span sp(e, s, 2);
    launch_noise(p, noise_dev, s);
  }
  if (p.table != nullptr) {
    // table evaluator: nothing leaves the tree kernel, one launch does the whole search
    Span sp(e, s, 0);
    launch_advance(p, 0, s);
  } else {
    const int sims = e->cfg.mcts_simulations;
    for (int it = 0; it <= sims; ++it) {
      {
        Span sp(e, s, 0);
        launch_advance(p, it, s);
      }
      if (it == sims) break;
      {
        Span sp(e, s, 1);
        launch_net(e->dev.prog.get(), 0, net_weights(e), p.leaf_boards, nullptr,
                   p.leaf_count + (it & 1), e->n_games, e->dev.leaf_logits.get(), e->dev.leaf_value.get(), nullptr, nullptr, s,
                   e->prec);
      }
    }
  }
  return NZ_OK;
}

static nz_status check_lockstep_call(nz_engine* e, const double* noise_dev, const double* uniforms_dev, bool need_uni) {
  if (e->n_slots != e->n_games)
    return fail(e, NZ_ERR_STATE, "the lock-step route needs n_slots == n_games (every game of the round in flight)");
  if (!e->have_net && !e->have_table) return fail(e, NZ_ERR_STATE, "no network: call nz_engine_set_weights first");
  if (e->cfg.training && (!noise_dev || (need_uni && !uniforms_dev)))
    return fail(e, NZ_ERR_ARG, "training search needs noise and uniforms");
  return NZ_OK;
}

nz_status nz_engine_move(nz_engine* e, const double* noise_dev, const double* uniforms_dev, void* stream) {
  if (!e) return NZ_ERR_ARG;
  nz_status st = check_lockstep_call(e, noise_dev, uniforms_dev, true);
  if (st != NZ_OK) return st;
  NZ_HIP(e, hipSetDevice(e->device));
  hipStream_t s = as_stream(stream);
  search_lockstep(e, noise_dev, s);
  {
    Span sp(e, s, 2);
    launch_finish_move(e->tp, uniforms_dev, nullptr, s);
  }
  NZ_HIP(e, hipGetLastError());
  return NZ_OK;
}

nz_status nz_engine_search(nz_engine* e, const double* noise_dev, void* stream) {
  if (!e) return NZ_ERR_ARG;
  nz_status st = check_lockstep_call(e, noise_dev, nullptr, false);
  if (st != NZ_OK) return st;
  NZ_HIP(e, hipSetDevice(e->device));
  search_lockstep(e, noise_dev, as_stream(stream));
  NZ_HIP(e, hipGetLastError());
  return NZ_OK;
}

nz_status nz_engine_apply(nz_engine* e, const int32_t* actions_dev, const double* uniforms_dev, void* stream) {
  if (!e) return NZ_ERR_ARG;
  if (e->n_slots != e->n_games)
    return fail(e, NZ_ERR_STATE, "the lock-step route needs n_slots == n_games (every game of the round in flight)");
  if (!actions_dev && e->cfg.training && !uniforms_dev)
    return fail(e, NZ_ERR_ARG, "a training engine choosing its own action needs uniforms");
  NZ_HIP(e, hipSetDevice(e->device));
  hipStream_t s = as_stream(stream);
  {
    Span sp(e, s, 2);
    launch_finish_move(e->tp, uniforms_dev, actions_dev, s);
  }
  NZ_HIP(e, hipGetLastError());
  return NZ_OK;
}

nz_status nz_engine_last_actions(nz_engine* e, int32_t* actions_dev, void* stream) {
  if (!e || !actions_dev) return NZ_ERR_ARG;
  NZ_HIP(e, hipSetDevice(e->device));
  launch_last_actions(e->tp, actions_dev, as_stream(stream));
  NZ_HIP(e, hipGetLastError());
  return NZ_OK;
}

nz_status nz_engine_live_games(nz_engine* e, int32_t* n_live_host, void* stream) {
  if (!e || !n_live_host) return NZ_ERR_ARG;
  hipStream_t s = as_stream(stream);
  NZ_HIP(e, hipMemcpyAsync(e->h_alive.get(), e->tp.alive, e->n_games * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  NZ_HIP(e, hipStreamSynchronize(s));
  int n = 0;
  for (int g = 0; g < e->n_games; ++g) n += e->h_alive[g] != 0;
  *n_live_host = n;
  return check_device_flag(e, s);
}

// The per-move draws of one game in the reference's order (SURVEY.md appendix A
// rule 13): gamma x n_children, then random() x 2 unless this is a softmax
// move, then at most one more random() inside np.random.choice.
static void draw_move(nz_rng* r, const nz_search_cfg& c, int move, int n_children, double* noise9, double* uni3) {
  nz_rng_gamma(r, c.root_dist_alpha, c.root_dist_beta, n_children, noise9);
  double u1 = 0.0, u2 = 0.0, u3 = 0.0;
  bool choice;
  if (move < c.number_of_softmax_moves) {
    choice = true;
  } else {
    u1 = nz_rng_double(r);
    u2 = nz_rng_double(r);
    choice = (u1 < c.epsilon_softmax_exploration) || (u2 < c.epsilon_random_exploration);
  }
  if (choice) u3 = nz_rng_double(r);
  uni3[0] = u1;
  uni3[1] = u2;
  uni3[2] = u3;
}

static void ensure_rngs(nz_engine* e) {
  if ((int)e->rngs.size() == e->n_games) return;
  for (nz_rng* r : e->rngs) nz_rng_destroy(r);
  e->rngs.assign(e->n_games, nullptr);
  for (int g = 0; g < e->n_games; ++g) e->rngs[g] = nz_rng_create(0);
}

// Lock-step play: one host round trip per move to learn each root's child count
// before drawing.  `seeds[g]` seeds game g's stream.
static nz_status play_lockstep(nz_engine* e, const uint32_t* seeds, void* stream) {
  if (e->n_slots != e->n_games)
    return fail(e, NZ_ERR_STATE, "the lock-step route needs n_slots == n_games (every game of the round in flight)");
  hipStream_t s = as_stream(stream);
  const int G = e->n_games;
  const nz_search_cfg& c = e->cfg;
  if (c.training) {
    ensure_rngs(e);
    for (int g = 0; g < G; ++g) nz_rng_seed(e->rngs[g], seeds[g]);
  }
  nz_status st = nz_engine_reset(e, stream);
  if (st != NZ_OK) return st;
  for (int move = 0; move < TTT_MAX_MOVES; ++move) {
    NZ_HIP(e, hipMemcpyAsync(e->h_children.get(), e->tp.n_root_children, G * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    NZ_HIP(e, hipMemcpyAsync(e->h_alive.get(), e->tp.alive, G * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    NZ_HIP(e, hipStreamSynchronize(s));
    int live = 0;
    for (int g = 0; g < G; ++g) live += e->h_alive[g] != 0;
    if (live == 0) break;
    if (c.training) {
      for (int g = 0; g < G; ++g)
        if (e->h_alive[g])
          draw_move(e->rngs[g], c, move, e->h_children[g], e->h_noise.get() + (size_t)g * TTT_ACTIONS, e->h_uniforms.get() + g * 3);
      NZ_HIP(e, hipMemcpyAsync(e->dev.noise.get(), e->h_noise.get(), (size_t)G * TTT_ACTIONS * sizeof(double), hipMemcpyHostToDevice, s));
      NZ_HIP(e, hipMemcpyAsync(e->dev.uniforms.get(), e->h_uniforms.get(), (size_t)G * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    }
    st = nz_engine_move(e, e->dev.noise.get(), e->dev.uniforms.get(), stream);
    if (st != NZ_OK) return st;
  }
  return check_device_flag(e, s);
}

nz_status nz_engine_play_lockstep(nz_engine* e, uint64_t base_seed, void* stream) {
  if (!e) return NZ_ERR_ARG;
  if (!e->have_net && !e->have_table) return fail(e, NZ_ERR_STATE, "no network: call nz_engine_set_weights first");
  NZ_HIP(e, hipSetDevice(e->device));
  std::vector<uint32_t> seeds(e->n_games);
  for (int g = 0; g < e->n_games; ++g) seeds[g] = (uint32_t)((base_seed + (uint64_t)g) & 0xffffffffu);
  return play_lockstep(e, seeds.data(), stream);
}

// Replay the games the persistent kernel flagged (their pre-drawn randomness did
// not fit) on a small lock-step engine and copy their records back.
static nz_status replay_desynced(nz_engine* e, const std::vector<int>& games, uint64_t base_seed, void* stream) {
  hipStream_t s = as_stream(stream);
  const int n = (int)games.size();
  if (e->fallback && e->fallback->n_games < n) {
    nz_engine_destroy(e->fallback);
    e->fallback = nullptr;
  }
  if (!e->fallback) {
    nz_engine* f = nullptr;
    nz_status st = nz_engine_create(&f, &e->cfg, &e->game, std::max(n, 16), e->device);
    if (st != NZ_OK) return fail(e, st, "fallback engine: %s", nz_last_error(nullptr));
    e->fallback = f;
  }
  nz_engine* f = e->fallback;
  f->borrowed_weights = e->weights_dev.get();
  f->prec = e->prec;                    // (the lock-step route runs the network kernel of the same mode)
  f->tp.table = e->tp.table;
  f->have_net = e->have_net;
  f->have_table = e->have_table;
  f->prog_host = e->prog_host;
  NZ_HIP(e, hipMemcpy(f->dev.prog.get(), &e->prog_host, sizeof(NetProgram), hipMemcpyHostToDevice));
  std::vector<uint32_t> seeds(f->n_games, 0u);
  for (int i = 0; i < n; ++i) seeds[i] = (uint32_t)((base_seed + (uint64_t)games[i]) & 0xffffffffu);
  nz_status st = play_lockstep(f, seeds.data(), stream);
  if (st != NZ_OK) return fail(e, st, "fallback replay: %s", f->error.c_str());
  const TreeParams &a = f->tp, &b = e->tp;
  for (int i = 0; i < n; ++i) {
    const size_t g = games[i];
#define ROW(field, per_game)                                                                               \
  NZ_HIP(e, hipMemcpyAsync(b.field + g * (per_game), a.field + (size_t)i * (per_game),                     \
                           (per_game) * sizeof(*a.field), hipMemcpyDeviceToDevice, s))
    ROW(hist_board, TTT_MAX_MOVES); ROW(hist_action, TTT_MAX_MOVES); ROW(hist_tree_size, TTT_MAX_MOVES);
    ROW(hist_children, TTT_MAX_MOVES); ROW(hist_bias, TTT_MAX_MOVES); ROW(hist_root_value_sum, TTT_MAX_MOVES);
    ROW(hist_visits, TTT_MAX_MOVES * TTT_ACTIONS); ROW(hist_prior, TTT_MAX_MOVES * TTT_ACTIONS);
    ROW(hist_value_sum, TTT_MAX_MOVES * TTT_ACTIONS);
    ROW(length, 1); ROW(outcome, 1); ROW(board, 1);
    ROW(sim_count, 1); ROW(exp_count, 1); ROW(sel_nodes, 1); ROW(sel_children, 1); ROW(new_nodes, 1);
#undef ROW
  }
  NZ_HIP(e, hipStreamSynchronize(s));
  return NZ_OK;
}

// every game's draws for a whole round into (noise [G][T][A], uniforms [G][T][3]), assuming the root of move m >= 1
// has 9 - m children (selfplay.hip); games are dealt to host threads
static void draw_round(nz_engine* e, uint64_t base_seed, double* noise, double* uniforms) {
  const int G = e->n_games;
  const nz_search_cfg& c = e->cfg;
  const int n_threads = std::max(1, std::min(16, (int)std::thread::hardware_concurrency()));
  auto work = [&](int t) {
    for (int g = t; g < G; g += n_threads) {
      nz_rng* r = e->rngs[g];
      nz_rng_seed(r, (uint32_t)((base_seed + (uint64_t)g) & 0xffffffffu));
      for (int m = 0; m < TTT_MAX_MOVES; ++m)
        draw_move(r, c, m, m == 0 ? 0 : TTT_ACTIONS - m, noise + ((size_t)g * TTT_MAX_MOVES + m) * TTT_ACTIONS,
                  uniforms + ((size_t)g * TTT_MAX_MOVES + m) * 3);
    }
  };
  if (G < 256 || n_threads == 1) {
    for (int t = 0; t < n_threads; ++t) work(t);
  } else {
    std::vector<std::thread> pool;
    for (int t = 0; t < n_threads; ++t) pool.emplace_back(work, t);
    for (auto& th : pool) th.join();
  }
}

nz_status nz_engine_play(nz_engine* e, uint64_t base_seed, void* stream) {
  return nz_engine_play_next(e, base_seed, 0, 0, stream);
}

nz_status nz_engine_play_next(nz_engine* e, uint64_t base_seed, int32_t have_next, uint64_t next_base_seed, void* stream) {
  if (!e) return NZ_ERR_ARG;
  if (!e->have_net && !e->have_table) return fail(e, NZ_ERR_STATE, "no network: call nz_engine_set_weights first");
  NZ_HIP(e, hipSetDevice(e->device));
  hipStream_t s = as_stream(stream);
  const int G = e->n_games;
  const nz_search_cfg& c = e->cfg;

  nz_status st = nz_engine_reset(e, stream);
  if (st != NZ_OK) return st;
  if (c.training) {
    ensure_rngs(e);
    const size_t GT = (size_t)G * TTT_MAX_MOVES;
    if (e->next_ready && e->next_seed == base_seed) {      // drawn under the previous round's kernel
      std::swap(e->h_game_noise, e->h_next_noise);
      std::swap(e->h_game_uniforms, e->h_next_uniforms);
    } else {
      draw_round(e, base_seed, e->h_game_noise.get(), e->h_game_uniforms.get());
    }
    e->next_ready = false;
    NZ_HIP(e, hipMemcpyAsync(e->dev.game_noise.get(), e->h_game_noise.get(), GT * TTT_ACTIONS * sizeof(double), hipMemcpyHostToDevice, s));
    NZ_HIP(e, hipMemcpyAsync(e->dev.game_uniforms.get(), e->h_game_uniforms.get(), GT * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  }
  {
    Span sp(e, s, 0);
    // (a packed engine that plays from a table has no packed program and never reaches the network phase)
    const bool packed = e->packed && e->have_net && e->packed_ready[e->tp.slots_per_wg];
    launch_selfplay(e->tp, packed ? e->packed_prog[e->tp.slots_per_wg].get() : e->dev.prog.get(), 0, net_weights(e),
                    c.training ? e->dev.game_noise.get() : nullptr, c.training ? e->dev.game_uniforms.get() : nullptr,
                    e->stamps ? e->dev.stamps.get() : nullptr, packed, s, e->prec);
  }
  NZ_HIP(e, hipGetLastError());
  if (c.training && have_next) {                            // the next round's draws, while the kernel runs
    draw_round(e, next_base_seed, e->h_next_noise.get(), e->h_next_uniforms.get());
    e->next_ready = true;
    e->next_seed = next_base_seed;
  }
  st = check_device_flag(e, s);
  if (st != NZ_OK) return st;
  if (c.training) {
    NZ_HIP(e, hipMemcpyAsync(e->h_desync.get(), e->tp.desync, G * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    NZ_HIP(e, hipStreamSynchronize(s));
    std::vector<int> bad;
    for (int g = 0; g < G; ++g)
      if (e->h_desync[g]) bad.push_back(g);
    if (!bad.empty()) {
      e->desync_total += (int64_t)bad.size();
      st = replay_desynced(e, bad, base_seed, stream);
      if (st != NZ_OK) return st;
    }
  }
  return NZ_OK;
}

nz_status nz_engine_phase_stamps(nz_engine* e, int32_t enable, double* out4_host) {
  if (!e) return NZ_ERR_ARG;
  if (out4_host) {
    const int blocks = selfplay_blocks(e->n_slots, e->tp.slots_per_wg);
    std::vector<unsigned long long> h((size_t)blocks * 8);
    NZ_HIP(e, hipSetDevice(e->device));
    NZ_HIP(e, hipDeviceSynchronize());
    NZ_HIP(e, hipMemcpy(h.data(), e->dev.stamps.get(), h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    double sum[4] = {0, 0, 0, 0};
    double max_total = 0;
    for (int b = 0; b < blocks; ++b) {
      for (int i = 0; i < 4; ++i) sum[i] += (double)h[b * 4 + i];
      max_total = std::max(max_total, (double)h[b * 4 + 3]);
    }
    out4_host[0] = sum[0] / blocks;              // mean tree/net cycles per workgroup
    out4_host[1] = sum[1] / std::max(sum[3], 1.0);   // share of ticks in the tree phase
    out4_host[2] = sum[2] / std::max(sum[3], 1.0);   // share of ticks in the net phase
    out4_host[3] = sum[3] / blocks / std::max(max_total, 1.0);   // mean / max workgroup lifetime
    out4_host[4] = sum[2] / std::max(sum[0], 1.0);   // shader-clock ticks per network phase
    out4_host[5] = sum[1] / std::max(sum[0], 1.0);   // shader-clock ticks per tree phase
    out4_host[6] = max_total;                        // ticks of the longest-lived workgroup
    out4_host[7] = (double)blocks;
    double fin = 0, exp = 0;
    for (int b = 0; b < blocks; ++b) {
      fin += (double)h[(size_t)blocks * 4 + b * 2];
      exp += (double)h[(size_t)blocks * 4 + b * 2 + 1];
    }
    out4_host[8] = fin / std::max(sum[0], 1.0);      // wave 0: ticks per cycle in end-of-move bookkeeping
    out4_host[9] = exp / std::max(sum[0], 1.0);      // simulations of the slowest row per cycle
    double passes = 0, sims = 0;
    for (int b = 0; b < blocks; ++b) {
      passes += (double)h[(size_t)blocks * 6 + b * 2];
      sims += (double)h[(size_t)blocks * 6 + b * 2 + 1];
    }
    out4_host[10] = passes / blocks;                 // network passes with a wave sitting out, per workgroup
    out4_host[11] = sims / blocks;                   // simulations run under network passes, per workgroup
  }
  e->stamps = enable != 0;
  return NZ_OK;
}

nz_status nz_engine_desync_count(const nz_engine* e, int64_t* count_host) {
  if (!e || !count_host) return NZ_ERR_ARG;
  *count_host = e->desync_total;
  return NZ_OK;
}

nz_status nz_engine_export(nz_engine* e, float* states, int32_t* visits, int32_t* actions, int32_t* lengths,
                           int32_t* outcomes, int32_t* tree_size, int32_t* n_children, double* bias, void* stream) {
  if (!e) return NZ_ERR_ARG;
  NZ_HIP(e, hipSetDevice(e->device));
  hipStream_t s = as_stream(stream);
  Span sp(e, s, 2);
  if (states) launch_export_states(e->tp, states, s);
  if (visits || actions || tree_size || n_children || bias)
    launch_export_visits(e->tp, visits, actions, tree_size, n_children, bias, s);
  if (lengths)
    NZ_HIP(e, hipMemcpyAsync(lengths, e->tp.length, e->n_games * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (outcomes)
    NZ_HIP(e, hipMemcpyAsync(outcomes, e->tp.outcome, e->n_games * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  NZ_HIP(e, hipGetLastError());
  return NZ_OK;
}

nz_status nz_engine_export_trace(nz_engine* e, double* child_prior, double* child_value_sum, double* root_value_sum,
                                 void* stream) {
  if (!e) return NZ_ERR_ARG;
  hipStream_t s = as_stream(stream);
  const size_t GT = (size_t)e->n_games * TTT_MAX_MOVES;
  if (child_prior)
    NZ_HIP(e, hipMemcpyAsync(child_prior, e->tp.hist_prior, GT * TTT_ACTIONS * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (child_value_sum)
    NZ_HIP(e, hipMemcpyAsync(child_value_sum, e->tp.hist_value_sum, GT * TTT_ACTIONS * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (root_value_sum)
    NZ_HIP(e, hipMemcpyAsync(root_value_sum, e->tp.hist_root_value_sum, GT * sizeof(double), hipMemcpyDeviceToDevice, s));
  return NZ_OK;
}

nz_status nz_engine_counters(nz_engine* e, int64_t* simulations_host, int64_t* expansions_host, void* stream) {
  if (!e) return NZ_ERR_ARG;
  hipStream_t s = as_stream(stream);
  std::vector<int32_t> a(e->n_games), b(e->n_games);
  NZ_HIP(e, hipMemcpyAsync(a.data(), e->tp.sim_count, a.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  NZ_HIP(e, hipMemcpyAsync(b.data(), e->tp.exp_count, b.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  NZ_HIP(e, hipStreamSynchronize(s));
  int64_t sa = 0, sb = 0;
  for (int g = 0; g < e->n_games; ++g) { sa += a[g]; sb += b[g]; }
  if (simulations_host) *simulations_host = sa;
  if (expansions_host) *expansions_host = sb;
  return NZ_OK;
}

// n_out values of {simulations, expansions, scored nodes, scored children, nodes created}; the caller says how many its
// array holds, so a caller built against an older header (four values) is never written past
nz_status nz_engine_counters_n(nz_engine* e, int64_t* out_host, int32_t n_out, void* stream) {
  if (!e || !out_host || n_out < 1 || n_out > 5) return NZ_ERR_ARG;
  hipStream_t s = as_stream(stream);
  const int32_t* src[5] = {e->tp.sim_count, e->tp.exp_count, e->tp.sel_nodes, e->tp.sel_children, e->tp.new_nodes};
  std::vector<int32_t> h(e->n_games);
  for (int i = 0; i < n_out; ++i) {
    NZ_HIP(e, hipMemcpyAsync(h.data(), src[i], h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    NZ_HIP(e, hipStreamSynchronize(s));
    int64_t sum = 0;
    for (int32_t v : h) sum += v;
    out_host[i] = sum;
  }
  return NZ_OK;
}

nz_status nz_engine_counters_ex(nz_engine* e, int64_t* out4_host, void* stream) {   // the first four, as first published
  return nz_engine_counters_n(e, out4_host, 4, stream);
}

nz_status nz_engine_net_flops(const nz_engine* e, double* flops_host) {
  if (!e || !flops_host) return NZ_ERR_ARG;
  *flops_host = e->algorithmic_flops_per_position;
  return NZ_OK;
}

nz_status nz_engine_net_matrix_flops(const nz_engine* e, double* bf16_flops_host, double* f32_flops_host) {
  if (!e || !bf16_flops_host || !f32_flops_host) return NZ_ERR_ARG;
  *bf16_flops_host = e->executed_bf16_flops_per_position;
  *f32_flops_host = e->executed_f32_flops_per_position;
  return NZ_OK;
}

nz_status nz_net_forward(nz_engine* e, const float* states_dev, int32_t batch, float* logits_dev, float* value_dev,
                         float* probs_dev, void* stream) {
  if (!e || !states_dev || !logits_dev || !value_dev) return NZ_ERR_ARG;
  if (!e->have_net) return fail(e, NZ_ERR_STATE, "no network: call nz_engine_set_weights first");
  if (batch <= 0) return NZ_OK;
  NZ_HIP(e, hipSetDevice(e->device));
  Span sp(e, as_stream(stream), 1);
  launch_net(e->dev.prog.get(), 0, net_weights(e), nullptr, states_dev, nullptr, batch, logits_dev,
             value_dev, probs_dev, nullptr, as_stream(stream), e->prec);
  NZ_HIP(e, hipGetLastError());
  return NZ_OK;
}

nz_status nz_net_forward_packed(nz_engine* e, const float* states_dev, int32_t batch, int32_t positions_per_pass,
                                float* logits_dev, float* value_dev, float* probs_dev, void* stream) {
  if (!e || !states_dev || !logits_dev || !value_dev) return NZ_ERR_ARG;
  if (!e->have_net) return fail(e, NZ_ERR_STATE, "no network: call nz_engine_set_weights first");
  if (e->prec == NZ_PREC_BF16)
    return fail(e, NZ_ERR_STATE, "the packed pass is float32 only: this engine is in plain-bf16 mode (nz_engine_precision)");
  if (batch <= 0) return NZ_OK;
  NZ_HIP(e, hipSetDevice(e->device));
  const NetProgram* prog = nullptr;
  const nz_status st = packed_program(e, positions_per_pass, &prog);
  if (st != NZ_OK) return st;
  Span sp(e, as_stream(stream), 1);
  launch_net_packed(prog, positions_per_pass, net_weights(e), states_dev, batch, logits_dev, value_dev, probs_dev,
                    as_stream(stream));
  NZ_HIP(e, hipGetLastError());
  return NZ_OK;
}

nz_status nz_net_forward_stamps(nz_engine* e, const float* states_dev, int32_t batch, float* logits_dev,
                                float* value_dev, double* ticks4_host) {
  if (!e || !states_dev || !logits_dev || !value_dev || !ticks4_host) return NZ_ERR_ARG;
  if (!e->have_net) return fail(e, NZ_ERR_STATE, "no network: call nz_engine_set_weights first");
  if (e->prec == NZ_PREC_BF16)
    return fail(e, NZ_ERR_STATE, "the stamped network kernel is float32 only: this engine is in plain-bf16 mode (nz_engine_precision)");
  NZ_HIP(e, hipSetDevice(e->device));
  const int blocks = (batch + 15) / 16;
  DevBuf<unsigned long long> stamps;
  if (!stamps.ensure((size_t)blocks * 4)) return fail(e, NZ_ERR_HIP, "device allocation failed");
  launch_net(e->dev.prog.get(), 0, net_weights(e), nullptr, states_dev, nullptr, batch, logits_dev, value_dev, nullptr, stamps.get(),
             nullptr);
  std::vector<unsigned long long> h((size_t)blocks * 4);
  hipError_t err = hipMemcpy(h.data(), stamps.get(), h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  if (err != hipSuccess) return fail(e, NZ_ERR_HIP, "stamp read-back failed: %s", hipGetErrorString(err));
  for (int i = 0; i < 4; ++i) {
    double sum = 0;
    for (int b = 0; b < blocks; ++b) sum += (double)h[(size_t)b * 4 + i];
    ticks4_host[i] = sum / blocks;
  }
  return NZ_OK;
}

// ---- the plain-bf16 mode ----------------------------------------------------------------------------------------------
nz_status nz_engine_precision(nz_engine* e, int32_t mode, int32_t* current) {
  if (!e) return NZ_ERR_ARG;
  if (mode != -1 && mode != NZ_PREC_FLOAT32 && mode != NZ_PREC_BF16)
    return fail(e, NZ_ERR_ARG, "precision mode %d: NZ_PREC_FLOAT32, NZ_PREC_BF16, or -1 to read", mode);
  if (mode != -1 && mode != e->prec) {
    e->prec = mode;
    // the pass choice: the plain-bf16 pass is the 16-column pass on a wave's own job list, so no wave sits a pass out
    // and no engine takes the packed pass, whatever nz_engine_create derived; float32 gets that back
    const bool plain = mode == NZ_PREC_BF16;
    e->packed = plain ? false : e->f32_packed;
    e->tp.burst_under_net = plain ? 0 : e->f32_burst;
    e->tp.sims_per_cycle = e->f32_sims_per_cycle;
    if (plain && !getenv("NZ_SIMS_PER_CYCLE")) e->tp.sims_per_cycle = 16;       // nz_engine_create's cap without the switch
    // the weights were packed for the other mode's stream: the engine is back to "no weights" (a table stays)
    if (e->have_net) {
      e->have_net = false;
      for (bool& ready : e->packed_ready) ready = false;
    }
  }
  if (current) *current = e->prec;
  return NZ_OK;
}

nz_status nz_net_forward_dump(nz_engine* e, const float* states_dev, int32_t batch, float* logits_dev, float* value_dev,
                              float* probs_dev, float* planes_dev, float* acts_dev, int32_t max_stages, float* vcells_dev,
                              int32_t* n_stages, void* stream) {
  if (!e || !states_dev || !logits_dev || !value_dev || !planes_dev || !acts_dev || !vcells_dev || max_stages < 0) return NZ_ERR_ARG;
  if (e->prec != NZ_PREC_BF16)
    return fail(e, NZ_ERR_STATE, "nz_net_forward_dump exists in plain-bf16 mode only (nz_engine_precision)");
  if (!e->have_net) return fail(e, NZ_ERR_STATE, "no network: call nz_engine_set_weights first");
  if (n_stages) *n_stages = e->prog_host.n_stages;
  if (batch <= 0) return NZ_OK;
  NZ_HIP(e, hipSetDevice(e->device));
  launch_net_dump(e->dev.prog.get(), net_weights(e), states_dev, batch, logits_dev, value_dev, probs_dev, planes_dev,
                  acts_dev, max_stages, vcells_dev, as_stream(stream));
  NZ_HIP(e, hipGetLastError());
  return NZ_OK;
}

nz_status nz_net_bf16_stream(const float* w, int32_t cout, int32_t cin, int32_t cin_main, int32_t k, uint32_t* words,
                             int64_t max_words, int64_t* n_main, int64_t* n_extra) {
  if (!w || !n_main || !n_extra || (!words && max_words > 0)) return NZ_ERR_ARG;
  if (cout <= 0 || cout > 64 || cin <= 0 || cin_main < 0 || cin_main > 64 || cin < cin_main || cin > cin_main + 4 || (k != 1 && k != 3)) {
    g_create_error = "nz_net_bf16_stream: a conv of at most 64 output and 64 main input channels, at most 4 input planes, k 1 or 3";
    return NZ_ERR_ARG;
  }
  std::vector<float> host((size_t)cout * cin * 9, 0.f), packed;
  for (size_t j = 0; j < (size_t)cout * cin; ++j)
    for (int t = 0; t < 9; ++t) host[j * 9 + t] = k == 3 ? w[j * 9 + t] : (t == 4 ? w[j] : 0.f);
  const PackedConv pc = pack_conv(host.data(), cout, cin, cin_main, packed, NZ_PREC_BF16);
  *n_main = pc.wx_off - pc.w_off;
  *n_extra = (int64_t)packed.size() - pc.wx_off;
  const int64_t n = std::min<int64_t>(max_words, (int64_t)packed.size() - pc.w_off);
  if (n > 0) memcpy(words, packed.data() + pc.w_off, (size_t)n * 4);
  return NZ_OK;
}

nz_status nz_net_program_convs(const nz_net_desc* net, int32_t recurrent_iterations, int32_t* conv_of_job, int32_t max_jobs,
                               int32_t* n_jobs) {
  if (!net || !n_jobs || (!conv_of_job && max_jobs > 0)) return NZ_ERR_ARG;
  NetLayout L;
  std::vector<PackedConv> convs;
  std::unique_ptr<NetProgram> pg(new NetProgram);
  std::vector<int> tensor_of[NET_WAVES_HOST];
  std::string bad = layout_only(net, recurrent_iterations, L, convs);
  double flops = 0.0;
  if (bad.empty()) bad = compile_net(net, L, convs, *pg, flops, tensor_of);
  if (!bad.empty()) {
    g_create_error = bad;
    return NZ_ERR_ARG;
  }
  int32_t n = 0;
  for (int w = 0; w < NET_WAVES_HOST; ++w)          // nz_net_program's rows: the jobs with work, wave by wave
    for (int j = 0; j < pg->n_jobs[w]; ++j) {
      if (pg->jobs[w][j].og == OG_NONE) continue;
      if (n < max_jobs) conv_of_job[n] = tensor_of[w][j];
      ++n;
    }
  *n_jobs = n;
  return NZ_OK;
}

// ---- evaluation matches (Tester.Test_using_agents, Testing/Tester.py:46-121) ------------------------------------------
// All matches of a round are at the same ply, so the mover's side and kind are known here: nine plies are enqueued
// back to back, finished matches are no-ops in every kernel, and the only synchronisation is the one after the tally.
nz_status nz_engine_match_play(nz_engine* side1, int32_t kind1, nz_engine* side2, int32_t kind2,
                               const uint32_t* agent_seeds1_host, const uint32_t* agent_seeds2_host,
                               const nz_ttt_match_result* out, void* stream) {
  return nz_engine_match_play_from(side1, kind1, side2, kind2, agent_seeds1_host, agent_seeds2_host, nullptr, out, stream);
}

// From start positions (all at one ply k, so the mover's side is still known here): plies k .. 8 are enqueued.
nz_status nz_engine_match_play_from(nz_engine* side1, int32_t kind1, nz_engine* side2, int32_t kind2,
                                    const uint32_t* agent_seeds1_host, const uint32_t* agent_seeds2_host,
                                    const uint32_t* start_boards_host, const nz_ttt_match_result* out, void* stream) {
  nz_engine* const eng[2] = {side1, side2};
  const int32_t kind[2] = {kind1, kind2};
  const uint32_t* const seeds[2] = {agent_seeds1_host, agent_seeds2_host};
  auto refuse = [&](nz_status code, const std::string& msg) {       // the message on every engine passed, and on NULL
    for (nz_engine* e : eng)
      if (e) e->error = msg;
    g_create_error = msg;
    return code;
  };
  for (int i = 0; i < 2; ++i) {
    const int k = kind[i];
    if (k != NZ_AGENT_MCTS && k != NZ_AGENT_POLICY && k != NZ_AGENT_RANDOM)
      return refuse(NZ_ERR_ARG, text("side %d: unknown agent kind %d", i + 1, k));
    if (k == NZ_AGENT_RANDOM) {
      if (eng[i]) return refuse(NZ_ERR_ARG, text("side %d: a random side takes no engine", i + 1));
      if (!seeds[i]) return refuse(NZ_ERR_ARG, text("side %d: a random side needs agent seeds, one per match", i + 1));
      continue;
    }
    const nz_engine* e = eng[i];
    if (!e) return refuse(NZ_ERR_ARG, text("side %d: an MCTS or policy side needs an engine", i + 1));
    if (e->cfg.training)
      return refuse(NZ_ERR_ARG, text("side %d: a training engine (evaluation agents do not explore: create it with training = 0)", i + 1));
    if (!e->cfg.keep_subtree) return refuse(NZ_ERR_ARG, text("side %d: keep_subtree = 0 is not supported", i + 1));
    if (!e->have_net && !e->have_table)
      return refuse(NZ_ERR_ARG, text("side %d: no network: call nz_engine_set_weights or nz_engine_set_table first", i + 1));
    if (e->n_slots != e->n_games)
      return refuse(NZ_ERR_ARG, text("side %d: a match engine needs n_slots == n_games (every match in flight)", i + 1));
  }
  if (!side1 && !side2) return refuse(NZ_ERR_ARG, "two random sides: one side must have an engine (it gives the number of matches)");
  if (side1 && side1 == side2 && !(kind1 == NZ_AGENT_POLICY && kind2 == NZ_AGENT_POLICY))
    return refuse(NZ_ERR_ARG, "both sides are the same engine: only two policy sides may share one (an MCTS side owns its trees)");
  if (side1 && side2 && side1->n_games != side2->n_games)
    return refuse(NZ_ERR_ARG, text("the engines hold %d and %d games: a match is one game on both", side1->n_games, side2->n_games));
  if (side1 && side2 && side1->device != side2->device)
    return refuse(NZ_ERR_ARG, text("the engines are on devices %d and %d", side1->device, side2->device));

  nz_engine* const host = side1 ? side1 : side2;
  const int n = host->n_games;
  int first_ply = 0;
  if (start_boards_host) {
    std::string msg;
    if (!check_start_boards(start_boards_host, n, true, &first_ply, msg)) return refuse(NZ_ERR_ARG, msg);
  }
  hipStream_t s = as_stream(stream);
  NZ_HIP(host, hipSetDevice(host->device));
  MatchArrays& m = host->match;
  if (!m.ensure((size_t)n)) return fail(host, NZ_ERR_HIP, "device allocation failed (match state)");
  host->match_kinds[0] = host->match_kinds[1] = -1;
  TttMatchArgs a = match_args(m, n);

  const uint32_t* start = nullptr;                           // the device copy every reset below reads
  if (start_boards_host) {
    NZ_HIP(host, hipMemcpyAsync(m.start.get(), start_boards_host, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    start = m.start.get();
  }
  nz_engine* mcts[2] = {nullptr, nullptr};
  for (int i = 0; i < 2; ++i)
    if (kind[i] == NZ_AGENT_MCTS) mcts[i] = eng[i];
  for (int i = 0; i < 2; ++i) {
    if (eng[i] && !(i == 1 && eng[1] == eng[0])) {
      // nz_engine_reset's launch with the start boards.  No hipSetDevice and no status of its own: an engine on
      // another device than the host engine's was refused above, and hipGetLastError is checked after the tally.
      Span sp(eng[i], s, 2);
      launch_reset(eng[i]->tp, start, s);
    }
    if (kind[i] == NZ_AGENT_RANDOM) {
      NZ_HIP(host, hipMemcpyAsync(m.seeds[i].get(), seeds[i], (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
      NZ_HIP(host, agent_seed_launch(m.seeds[i].get(), a.mt_keys[i], a.mt_pos[i], n, s));
    }
  }
  ttt_match_reset_launch(a, start, s);

  for (int ply = first_ply; ply < TTT_MAX_MOVES; ++ply) {
    const int mv = ply & 1;                                  // side 1 moves for player 1, the first mover
    for (nz_engine* e : mcts)
      if (e) search_lockstep(e, nullptr, s);                 // the mover's choose_action, the opponent's update_subtree
    if (kind[mv] == NZ_AGENT_MCTS) {
      launch_finish_move(mcts[mv]->tp, nullptr, nullptr, s);
      launch_last_actions(mcts[mv]->tp, a.forced, s);
      if (mcts[mv ^ 1]) launch_finish_move(mcts[mv ^ 1]->tp, nullptr, a.forced, s);
    } else {
      const float* table = nullptr;
      if (kind[mv] == NZ_AGENT_POLICY) {
        const nz_engine* pe = eng[mv];
        table = pe->tp.table;
        if (!table) {                                        // the stand-alone network route (nz_net_forward)
          ttt_state_image_launch(a, s);
          launch_net(pe->dev.prog.get(), 0, net_weights(pe), nullptr, a.states, nullptr, n, m.logits.get(), m.value.get(),
                     m.probs.get(), nullptr, s, pe->prec);
        }
      }
      ttt_agent_move_launch(a, mv, kind[mv], table, s);
      for (nz_engine* e : mcts)
        if (e) launch_finish_move(e->tp, nullptr, a.forced, s);
    }
    ttt_match_step_launch(a, s);
  }

  NZ_HIP(host, hipMemsetAsync(m.tally.get(), 0, 8 * sizeof(unsigned long long), s));
  ttt_match_tally_launch(a, mcts[0] ? mcts[0]->tp.error_flag : nullptr, mcts[1] ? mcts[1]->tp.error_flag : nullptr,
                         m.tally.get(), s);
  NZ_HIP(host, hipGetLastError());
  NZ_HIP(host, hipMemcpyAsync(m.h_tally.get(), m.tally.get(), 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  if (out) {
    const size_t nt = (size_t)n * TTT_MAX_MOVES * sizeof(int32_t);
    if (out->actions) NZ_HIP(host, hipMemcpyAsync(out->actions, a.actions, nt, hipMemcpyDeviceToDevice, s));
    if (out->lengths) NZ_HIP(host, hipMemcpyAsync(out->lengths, a.length, n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (out->outcomes) NZ_HIP(host, hipMemcpyAsync(out->outcomes, a.outcome, n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    for (int i = 0; i < 2; ++i) {
      if (out->agent_actions[i]) NZ_HIP(host, hipMemcpyAsync(out->agent_actions[i], a.agent_actions[i], nt, hipMemcpyDeviceToDevice, s));
      if (out->agent_n_legal[i]) NZ_HIP(host, hipMemcpyAsync(out->agent_n_legal[i], a.agent_n_legal[i], nt, hipMemcpyDeviceToDevice, s));
    }
  }
  NZ_HIP(host, hipStreamSynchronize(s));
  const unsigned long long* t = m.h_tally.get();
  if (t[5] || t[6])
    return fail(host, NZ_ERR_OVERFLOW, "device check failed (side-1 flag %llu, side-2 flag %llu: 1 = tree arena full, 2 = visit table "
                                       "too short, 4 = move finished before its search, 8 = forced action is not legal)", t[5], t[6]);
  if (t[4])
    return fail(host, NZ_ERR_STATE, "internal: a match's error word is set (%llu: 1 = randint rejection cap, 2 = no empty cell, "
                                    "4 = the mover's action is not an empty cell)", t[4]);
  if (out && out->tally4_host)
    for (int i = 0; i < 4; ++i) out->tally4_host[i] = (int64_t)t[i];
  host->match_kinds[0] = kind1;
  host->match_kinds[1] = kind2;
  return NZ_OK;
}

nz_status nz_engine_match_streams(nz_engine* e, int32_t side, uint32_t* keys_host, int32_t* pos_host) {
  if (!e || side < 0 || side > 1 || !keys_host || !pos_host) return fail(e, NZ_ERR_ARG, "bad argument");
  if (e->match_kinds[side] != NZ_AGENT_RANDOM)
    return fail(e, NZ_ERR_STATE, "side %d of this engine's last match round was no random side", side + 1);
  NZ_HIP(e, hipSetDevice(e->device));
  NZ_HIP(e, hipDeviceSynchronize());
  NZ_HIP(e, hipMemcpy(keys_host, e->match.mt_keys[side].get(), (size_t)e->n_games * MT_N * sizeof(uint32_t), hipMemcpyDeviceToHost));
  NZ_HIP(e, hipMemcpy(pos_host, e->match.mt_pos[side].get(), (size_t)e->n_games * sizeof(int32_t), hipMemcpyDeviceToHost));
  return NZ_OK;
}

nz_status nz_engine_policy_actions(nz_engine* e, const uint32_t* boards_host, int32_t n, int32_t* actions_dev, void* stream) {
  if (!e || !boards_host || !actions_dev)
    return fail(e, NZ_ERR_ARG, "nz_engine_policy_actions: NULL %s", !e ? "engine" : !boards_host ? "boards" : "actions");
  if (n <= 0 || n > e->n_games) return fail(e, NZ_ERR_ARG, "%d positions: an engine of %d games takes 1 .. %d", n, e->n_games, e->n_games);
  if (!e->have_net && !e->have_table)
    return fail(e, NZ_ERR_ARG, "no network: call nz_engine_set_weights or nz_engine_set_table first");
  std::string msg;
  if (!check_start_boards(boards_host, n, false, nullptr, msg)) return fail(e, NZ_ERR_ARG, "%s", msg.c_str());
  hipStream_t s = as_stream(stream);
  NZ_HIP(e, hipSetDevice(e->device));
  MatchArrays& m = e->match;
  if (!m.ensure((size_t)e->n_games)) return fail(e, NZ_ERR_HIP, "device allocation failed (match state)");
  e->match_kinds[0] = e->match_kinds[1] = -1;                // the match state is overwritten
  TttMatchArgs a = match_args(m, n);
  NZ_HIP(e, hipMemcpyAsync(m.start.get(), boards_host, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  ttt_match_reset_launch(a, m.start.get(), s);
  const float* table = e->tp.table;
  if (!table) {
    ttt_state_image_launch(a, s);
    launch_net(e->dev.prog.get(), 0, net_weights(e), nullptr, a.states, nullptr, n, m.logits.get(), m.value.get(), m.probs.get(),
               nullptr, s, e->prec);
  }
  // The mover runs as side 0 whoever is to move: only a.forced is read here.  Its by-ply rows (agent_actions[0] /
  // agent_n_legal[0]) are written too, into a match state declared overwritten above.  A playable position has an
  // empty cell, so forced is set for every one.
  ttt_agent_move_launch(a, 0, NZ_AGENT_POLICY, table, s);
  NZ_HIP(e, hipGetLastError());
  NZ_HIP(e, hipMemcpyAsync(actions_dev, a.forced, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  return NZ_OK;
}

nz_status nz_engine_profile(nz_engine* e, int32_t enable) {
  if (!e) return NZ_ERR_ARG;
  e->spans.clear();
  e->profile = enable != 0;
  return NZ_OK;
}

nz_status nz_engine_profile_read(nz_engine* e, double* ms_host, int64_t* launches_host, int64_t* net_positions_host) {
  if (!e) return NZ_ERR_ARG;
  NZ_HIP(e, hipSetDevice(e->device));
  NZ_HIP(e, hipDeviceSynchronize());
  double ms[3] = {0, 0, 0};
  int64_t n[3] = {0, 0, 0};
  for (auto& sp : e->spans) {
    float t = 0.f;
    NZ_HIP(e, hipEventElapsedTime(&t, sp.a.get(), sp.b.get()));
    ms[sp.cls] += t;
    n[sp.cls] += 1;
  }
  for (int i = 0; i < 3; ++i) {
    if (ms_host) ms_host[i] = ms[i];
    if (launches_host) launches_host[i] = n[i];
  }
  if (net_positions_host) *net_positions_host = 0;
  return NZ_OK;
}

}  // extern "C"
