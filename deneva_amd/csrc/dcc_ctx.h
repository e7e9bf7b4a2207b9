// dcc_ctx: the per-process, per-device engine context behind the C ABI.
// Replaces the reference's global OptCC singleton (`occ_man`,
// system/global.cpp:42) and owns every device workspace so that a validation
// call performs no allocation once warmed up.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "dcc.h"
#include "occ_history.h"

namespace dcc {
struct SwShard;  // occ_kernels.h: one key-sharded sweep level's serial range
struct Slot;     // dcc_device.h: one slot of the per-epoch hash table
}

struct dcc_ctx;


// A grow-only device allocation, freed with its owner: moving hands the
// memory over (the target's own is freed first), copying is not possible.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) {
    o.p = nullptr;
    o.cap = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      cap = o.cap;
      o.p = nullptr;
      o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  int ensure(dcc_ctx* c, size_t bytes, const char* what);
  void release();  // free now (a table that is dropped or replaced)
};

// A persistent row table (rowtab.h, where the methods and the kernels are):
// 2^bits 32-byte slots {key, a, b}, linear probing with the owning engine's
// probe policy P (dcc_device.h), at most half full.  set / get take host
// arrays; the engines' epochs enter rows with their own kernels and add what
// those counted to `rows`.
struct RowTab {
  const char* name;   // the owning engine, for messages
  DevBuf buf, ctl;    // the slots; {error word, rows a call added}
  uint32_t bits = 0;  // log2 slots (0: no table yet)
  uint64_t rows = 0;  // rows in the table
  uint32_t mask() const { return (uint32_t)((1ull << bits) - 1); }
  uint64_t size() const { return rows; }
  template <class P>
  int reserve(dcc_ctx* ctx, uint64_t want);  // room for `want` rows (rehash on growth)
  int clear(dcc_ctx* ctx);
  template <class P>
  int set(dcc_ctx* ctx, const uint64_t* keys, const uint64_t* a, const uint64_t* b, uint64_t n);
  template <class P>
  int get(dcc_ctx* ctx, const uint64_t* keys, uint64_t* a, uint64_t* b, uint64_t n);
};

// The workspaces of a sorted-segment epoch (seg_rounds.h):
// one set for TIMESTAMP, MVCC and WAIT_DIE, whose epochs and release use the
// same ten arrays with the same element sizes.  Nothing in them lives across
// calls: every call clears the counters and the tile flags it reads and
// writes every other word before it reads it; the rows, the version store
// and the lock state are elsewhere.  The sharing depends on that.
struct SegWork {
  static constexpr uint64_t TILE = 1024;    // accesses per scan tile (TS_TILE, WD_TILE)
  static constexpr uint32_t C_WORDS = 84;   // counter words (>= TS_C_WORDS, LV_C_WORDS)
  static constexpr size_t AGG_BYTES = 40;   // a tile aggregate (sizeof(Tq), sizeof(Wq))
  DevBuf misc;               // counters, the ring of undecided counts
  DevBuf stp;                // [n] txn words
  DevBuf arec;               // [nnz] the record of every access
  DevBuf k[2], v[2];         // the sort's ping-pong keys / values (access indices)
  DevBuf stxn, sinfo, sts;   // sorted txns / record words / timestamps
  DevBuf agg;                // [2 * tiles] tile aggregates, then their exclusive prefixes
  DevBuf tdone;              // [tiles] tile flags
  // room for n txns and nnz accesses; the per-access arrays of the sorted side
  // in whole tiles (k_ts_scan loads 16 bytes per lane)
  int reserve(dcc_ctx* ctx, uint64_t n, uint64_t nnz);
};

// A batch as device pointers (aliases the caller's or the ctx's staging).
struct DevBatch {
  uint64_t n = 0, nnz = 0;
  const uint32_t* off = nullptr;
  const uint64_t* keys = nullptr;
  const uint8_t* acctype = nullptr;
  const uint64_t* start_tn = nullptr;
  const uint64_t* finish_tn = nullptr;
  const uint64_t* order = nullptr;
};

struct dcc_comm_state;  // RCCL communicator (dcc_comm.hip)
struct dcc_multi;       // single-process multi-GPU context (dcc_multi.cpp)

// One level of the device OCC history (occ_history.h): flat (key, tn) pairs in
// append order and, once built, the pairs sorted by (key, tn) with the key
// table.
// The delta level also takes the epochs' appends as chains in its table
// (occ_history.h HistInsert), so an epoch's append needs no rebuild.
struct HistStore {
  DevBuf fk, ft;            // flat pairs
  DevBuf skey, stn, hash;   // built level
  DevBuf bm;                // key bitmap of the built level (occ_history.h HIST_BM_LOG)
  DevBuf nx, tcnt;          // delta: chain links per flat pair; the table's overflow flag
  uint64_t m = 0;           // pairs
  uint32_t hbits = 0;
  bool built = true;        // the built level (with its chains) holds every flat pair
  bool mono = true;         // append order is tn order within every key
  uint64_t max_tn = 0;      // largest tn appended
  uint64_t min_tn = ~0ull;  // smallest tn appended
  uint64_t max_key = 0;     // largest key appended (radix passes of the build)
  bool chained = false;     // the delta level
  bool overflowed = false;  // a key landed past HIST_WALK: the next build doubles the table
  uint64_t last_app = 0;    // delta: pairs the last epoch appended (table headroom)
  // empty the level, keeping its buffers (the next build clears its table)
  void reset() {
    m = 0;
    built = false;
    mono = true;
    max_tn = 0;
    min_tn = ~0ull;
    max_key = 0;
  }
};

// One OCC (sub-)batch: txn i has accesses [off[i], off[i+1]) of keys/acctype
// and the state byte state[i]; nnz bounds off[n], w_bound its write count.
struct SubProb {
  uint64_t n = 0, nnz = 0, w_bound = 0;
  const uint32_t* off = nullptr;
  const uint64_t* keys = nullptr;
  const uint8_t* acctype = nullptr;
  uint8_t* state = nullptr;
  uint8_t* hasw = nullptr;   // has-write bytes out
  bool hasw_global = false;  // hasw is the epoch's (all-reduced when sharded)
};
struct PeelInfo {
  uint64_t prefix = 0, survivors = 0;
};
// Dense survivor sub-batch of one peel level.
struct SubBufs {
  DevBuf tid, off, keys, acctype, state;
};

// The device-resident abort queue (abortq.hip).  Two CSR pools with their
// per-txn arrays: pushes append to pool `cur`, a pop compacts the kept entries
// into the other one and swaps.  Pool order is seq (push) order.
struct dcc_abortq {
  dcc_ctx* owner = nullptr;  // the creating context (a multi-GPU one runs the work on rank 0)
  dcc_abortq_params P{};
  struct Pool {
    DevBuf off, keys, at, src, cnt, due;
  } pool[2];
  DevBuf sk[2], sv[2], scratch;  // (due, pool index) pairs of the sort (ping-pong), its counts
  DevBuf ctl, part;              // control words; tile pairs of the pop's three compactions
  DevBuf st_cnt, st_out;         // cnt_in / the outputs of a host call
  int cur = 0;
  uint64_t n = 0, nnz = 0;  // parked txns / accesses
  uint64_t seq = 0;         // txns pushed over the queue's life
  uint64_t due_lo = ~0ull;  // a lower bound of every parked due: the smallest `now` pushed
                            // with since the queue was last empty
};

// The NO_WAIT lock table that lives across epochs (locktab.hip): Row_lock's
// (lock_type, owner_cnt) per row in an open-addressing table of n_slots
// 16-byte slots.  A released row keeps its slot, so the host tracks the slots
// in use next to the rows held and rebuilds into the other buffer when an
// epoch's requests would push the table past half full.
struct dcc_locktab {
  dcc_ctx* owner = nullptr;  // the creating context (a multi-GPU one runs the work on rank 0)
  dcc_locktab_params P{};
  DevBuf tab[2];                    // the table and the rebuild's target
  DevBuf ctl;                       // control words
  DevBuf st_keys, st_type, st_cnt;  // the outputs of a host export
  DevBuf st_rc;                     // rc of a host release
  int cur = 0;
  uint64_t n_slots = 0;
  uint64_t slots_used = 0;  // keys in the current buffer
  uint64_t rows_held = 0;   // rows with owner_cnt > 0
  uint64_t holds = 0;       // the sum of all owner_cnt
  uint64_t rebuilds = 0;
  double pass_ms[3] = {};   // seed / grant / rebuild of the last profiled epoch or acquire
  bool rebuilt = false;     // the call in flight rebuilt (pev[7] .. pev[0] is its time)
};

// What the table's passes of a lock epoch read of it (nowait.hip fills it in).
struct LtEpoch {
  uint64_t n = 0;
  const uint32_t* off = nullptr;
  const uint64_t* keys = nullptr;
  const uint8_t* at = nullptr;
  const uint32_t* sid = nullptr;   // per-epoch slot id of every request
  const uint8_t* state = nullptr;  // decided state bytes
  dcc::Slot* tab = nullptr;        // the per-epoch table
  uint32_t lp = 0;                 // log2 lanes per txn
  const uint32_t* err = nullptr;   // the epoch's error word
  unsigned grid = 1;
  uint32_t mask = 0;   // the per-epoch table's
  int level = 0;       // ISO_SER / ISO_RC / ISO_RU (nowait_lanes.h)
};

struct dcc_ctx {
  int device = 0;
  int n_cu = 256;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool profiling = false;
  uint64_t recheck_max = 16384;   // fold the kill wave into rounds with lists <= this
  uint32_t batch_max = 8;       // rounds enqueued between host synchronisations
  bool bars_used = false;       // this epoch's rounds used grid-barrier words
  int solver = 0;               // 0 auto (= 3), 1 fixed-point rounds, 3 sweep
  bool use_sweep() const { return solver != 1; }
  bool ro_split = true;           // DCC_OPT_RO_SPLIT
  bool ro_on = false;             // this epoch splits read-only txns off (sweep, one GPU)
  uint32_t wt_bits = 18;          // committed-writer table slots (WT_BITS_DEFAULT; grows after an overflow)
  uint32_t wf_bits = 0;           // fallback table (k_sw_wall) slots
  uint32_t sw_levels = 0;          // DCC_OPT_SWEEP_LEVELS (0: auto)
  uint32_t sw_mode = 1;            // this epoch's level schedule (occ_driver.hip sw_pmax)
  uint32_t sw_l1_last = ~0u;       // level-1 list length of the last one-GPU split epoch
  bool sw_debug = false;        // DCC_SW_DEBUG: per-tile clock stamps of the serial pass       // sweep levels enqueued between host synchronisations
  hipEvent_t pev[8] = {};  // phase boundary events (profiling only)
  std::string last_error;
  void* hmisc = nullptr;  // pinned host mirror of `misc`
  void* hpart = nullptr;  // pinned host mirror of `part`
  // the sweep epoch's captured launch sequence (occ_epoch) and what it was
  // captured with; buf_gen counts workspace reallocations
  struct GraphKey {
    const void *off, *keys, *acc;
    uint64_t n, nnz;
    const void* out_rc;
    bool dev_out;
    uint32_t levels;
    uint64_t gen;
    const void *start_tn, *finish_tn, *out_tn;
    uint32_t fin;  // want tn | append << 1 | window check << 2
    bool operator==(const GraphKey& o) const {
      return off == o.off && keys == o.keys && acc == o.acc && n == o.n && nnz == o.nnz &&
             out_rc == o.out_rc && dev_out == o.dev_out && levels == o.levels && gen == o.gen &&
             start_tn == o.start_tn && finish_tn == o.finish_tn && out_tn == o.out_tn && fin == o.fin;
    }
  };
  hipGraphExec_t graph_exec = nullptr;
  // the Calvin epoch's launch sequence after its prep read-back (calvin.hip):
  // captured the second time a shape is seen, replayed while it repeats
  struct CvGraphKey {
    const void *off, *keys, *acc, *order, *grp, *rc;
    uint64_t n, nnz, gen;
    uint32_t ulen, have_seq, bucket;
    uint8_t kp[112], op[112];  // KeyPack images (memcmp)
  };
  hipGraphExec_t cv_graph_exec = nullptr;
  CvGraphKey cv_graph_key{}, cv_seen_key{};
  bool cv_seen = false;
  bool cv_last_sorted = false, cv_last_bucket = false;  // the last Calvin epoch's order / path
  uint64_t cv_spec_miss = 0;  // speculative Calvin replays whose prep results differed
  GraphKey graph_key{};
  uint64_t buf_gen = 0;
  void* hmisc_dev = nullptr;  // device-visible addresses of the two (k_gather targets)
  void* hpart_dev = nullptr;
  // per-epoch values of a captured OCC epoch (dcc::OccDyn at offset 0, written
  // by the host before each launch) and the central_finish totals (offset
  // HDYN_TOTALS, written by the device); pinned
  void* hdyn = nullptr;
  void* hdyn_dev = nullptr;
  static constexpr size_t HDYN_TOTALS = 256, HDYN_BYTES = 512;

  // device workspaces (grow-only)
  DevBuf misc;                                   // counters / error words
  DevBuf part;                                   // per-block partial reductions
  DevBuf off, keys, acctype, start_tn, finish_tn, order;  // staged host batch
  DevBuf nar_keys, nar_at, nar_tn;                 // compact forms before widening (host batches)
  DevBuf table;                                  // Slot[cap]
  DevBuf state, hasw, rc, stat;                  // per-txn bytes
  DevBuf cflag, bsum, tn;                        // commit-tn scan
  DevBuf dyn, fin_part;                          // OccDyn (device copy), central_finish block counts
  DevBuf gst;                                    // sharded per-txn status
  DevBuf hasw_scr;                               // round-solver hand-off
  DevBuf sw_ctl, sw_status, sw_ckeys, sw_dbg;            // sweep solver: level control, look-back, C
  DevBuf sw_rec, sw_rk, sw_gtab, sw_fw, sw_aent, sw_mg;
  DevBuf sw_rflag, sw_ro, sw_wtab, sw_cw, sw_wtab_big;  // read-only split: survivor bits, RO
                                                        // list, writer tables, committed writers
  DevBuf sw_xcnt, sw_xsend, sw_xrec, sw_mcnt, sw_moff, sw_mkeys, sw_mat, sw_kill;  // key-sharded sweep  // sweep tile records
  SubBufs sw_list[2];                            // sweep level lists (ping-pong)
  DevBuf l_tid[2], l_coff[2], l_cent[2];         // ping-pong undecided lists
  // OCC history (occ.h:62-64) on the device: base + delta levels
  HistStore hs[2];
  uint64_t hist_merge_min = 65536;  // DCC_OPT_HIST_MERGE
  DevBuf h_K[2], h_V[2], h_scr, h_bsum;          // level-build sort buffers, append scan
  DevBuf h_bm;                                   // key bitmap of both levels (window check)
  bool h_bm_stale = true;                        // h_bm is not B.bm | D.bm
  uint32_t fin_tag = 0;                          // k_fin's look-back tag of the last epoch
  DevBuf perm, calvin_a, calvin_b, calvin_c, calvin_d;  // Calvin workspaces
  DevBuf cv_scratch, cv_agg, cv_group, cv_wave, cv_pgx, cv_gsx, cv_gsize, cv_done, cv_maxl, cv_cwmax, cv_cwpos, cv_cwmark, cv_cwhot, cv_cwpa, cv_cwoa, cv_cwhelp, cv_cwrec2;
  DevBuf cv_seq_b, cv_ok, cv_len, cv_off2, cv_tsum;
  DevBuf held_keys, held_at;  // held rows of a host call (Calvin / NO_WAIT: stage_held)
  DevBuf cb_e, cb_out, cb_cnt, cb_small;           // Calvin bucket path (calvin_bucket.h)
  DevBuf snap_top, snap_aoff, snap_aidx, snap_cnt;  // captured-snapshot validation
  RowTab mt_rows{"maat"};                        // MaaT row table: {key, last read, last write}
  uint64_t mt_new_last = 0;                      // rows the last epoch added (table sizing)
  uint64_t mt_full_redo = 0;                     // epochs run again on a bigger row table
  DevBuf mt_misc, mt_slot, mt_sval, mt_slot2, mt_sval2, mt_sfl, mt_stx, mt_txn, mt_agg;
  DevBuf mt_sflB, mt_stxB, mt_k1, mt_tcnt, mt_ul;
  DevBuf mt_lb;          // fused round scan: look-back status per tile (k_mt_round)
  DevBuf mt_ptab;        // prefix level: per-row commit bounds of the prefix (MtPTab)
  uint32_t mt_tag = 0;   // its round tag (monotone; the buffer is zeroed when it wraps)
  // GPU index (index.hip): key table, newest insert ordinal per key, rows
  DevBuf ix_keys, ix_ord, ix_rows, ix_cnt, wv_buf, ix_scr, wv_hbuf, wv_obuf;
  // NO_WAIT lock epoch (nowait.hip): counters, slot id per request, undecided
  // lists (ping-pong), conflict ordinals of a host call
  DevBuf nw_misc, nw_sid, nw_list, nw_conf;
  // select by decision (select.hip): control words, tile pairs; rc, src_in
  // and the output arrays of a host call
  DevBuf sel_misc, sel_part, sel_rc, sel_src, sel_out;
  // abort queues created on this context and not yet destroyed (freed with it)
  std::vector<std::unique_ptr<dcc_abortq>> abortqs;
  uint32_t ix_bits = 0;
  uint64_t ix_nkeys = 0, ix_nrows = 0;
  double ix_last_ms = 0;
  // commit counter tnc (occ.h:67)
  uint64_t tnc = 0;

  dcc_comm_state* comm = nullptr;
  dcc_multi* multi = nullptr;  // non-null: this context drives per-GPU sub-contexts
  int comm_ranks() const;
  bool sharded() const;    // the key-sharded paths run (ranks > 1, or a one-rank RCCL clique)
  bool comm_solo = false;  // DCC_OPT_COMM_SOLO
  int comm_allreduce_max_u8(uint8_t* dev, uint64_t n);  // in place, on `stream`
  // every rank's `bytes` from send into recv[rank * bytes ...], on `stream`
  int comm_allgather_u8(const uint8_t* send, uint8_t* recv, uint64_t bytes);
  int comm_rank() const;

  int fail(int code, const char* fmt, ...);
  int hip_fail(hipError_t e, const char* what);
  int reserve_occ(uint64_t n, uint64_t nnz, uint64_t nnz_w, uint32_t tw);
  void list_geometry(uint64_t n, uint32_t tw, uint64_t& seg_ts, uint64_t& seg_es) const;
  static uint64_t table_capacity(uint64_t nnz_w);
  // device history (occ_history.h / dcc_ctx.hip)
  uint64_t hist_size() const { return hs[0].m + hs[1].m; }
  int hist_grow_flat(HistStore& h, uint64_t need);
  dcc::HistInsert hist_insert_args(HistStore& h);
  void hist_note(HistStore& h, uint64_t lo_tn, uint64_t hi_tn);
  int hist_build(HistStore& h);
  int hist_prepare();  // merge policy + rebuild: call before a window check
  dcc::HistView hist_view() const;
  int hist_append_epoch(const DevBatch& d, const uint64_t* tn_dev, uint64_t nnz_w, uint64_t n_cw);
  // scan_offsets: the O(n) host pass over a host batch's offsets (the sweep
  // validates them on the device instead, inside its level-0 launch)
  int check_batch(const dcc_batch* b, bool scan_offsets = true);
  int stage_batch(const dcc_batch* b, DevBatch& d);
  // One input array of a call as a device array: a host array (`dev` false)
  // is copied into `buf` on `stream`, a device array is read in place.
  template <typename T>
  int stage(DevBuf& buf, const T* src, size_t bytes, bool dev, const char* what, const T*& out) {
    if (dev) {
      out = src;
      return DCC_OK;
    }
    if (int e = buf.ensure(this, bytes, what)) return e;
    if (bytes) {
      const hipError_t he = hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, stream);
      if (he != hipSuccess) return hip_fail(he, what);
    }
    out = (const T*)buf.p;
    return DCC_OK;
  }
  // the held rows of a Calvin / NO_WAIT epoch (none: null arrays)
  int stage_held(const dcc_calvin_held* held, bool dev, const uint64_t*& keys, const uint8_t*& at);
  int device_prep(const DevBatch& d, uint32_t& maxlen, uint64_t& nnz_w, uint64_t p = 0,
                  uint64_t* nnz_w_prefix = nullptr);
  int read_partials(size_t bytes);
  int occ_epoch(const dcc_batch* b, uint8_t* out_rc, uint64_t* out_tn, dcc_stats* st);
  // The epoch in two halves (occ_pipe.cpp overlaps epochs of several lane
  // contexts): begin enqueues; with `async` and a replayable graph it returns
  // right after the graph launch (run.pending) and end synchronises.
  struct OccRun {
    uint64_t n_txn = 0;
    uint32_t flags = 0;
    uint8_t* out_rc = nullptr;
    uint64_t* out_tn = nullptr;
    DevBatch d;
    bool sh = false, dev_out = false, defer = false, sweep = false, want_tn = false;
    bool app = false, hist_on = false;  // history append (central_finish) / window check
    bool whole = false;                 // key-sharded rank holding the whole batch (DCC_SHARD_SELF)
    DevBatch full;                      // that batch
    bool replay = false, capturing = false, pending = false, active = false;
    uint32_t glv = 0, maxlen = 0, rounds = 0, handoffs = 0;
    uint64_t nnz_w = 0;
    int next_level = 0, serial_tail = -1;
    uint8_t* rc_dev = nullptr;
    uint32_t* cf = nullptr;
    uint64_t* tn_dev = nullptr;
    PeelInfo info;
    GraphKey gkey{};
    dcc_stats S;
    double t_wall0 = 0;
    uint64_t n_cw = 0;  // committed writers of the finished epoch (tnc advance)
    uint32_t fin_runs = 0;  // central_finish launches (a second one after more levels)
    bool fin_later = false; // pipeline lane: central_finish runs at completion (pipe_finish)
  };
  OccRun run;
  int occ_begin(const dcc_batch* b, uint8_t* out_rc, uint64_t* out_tn, bool async, bool fin_later = false);
  // the central_finish of lane `l`'s completed epoch (decided with fin_later):
  // commit tn from this context's tnc, the history append into this
  // context's delta level -- run by the parent in submit order (occ_pipe.cpp)
  // chained: other chained epochs may be in flight behind it (their finishes
  // write into the delta level): no merge, rebuild or growth here
  int pipe_finish(dcc_ctx* l, bool chained = false);
  // Chained central_finish (occ_pipe.cpp, DCC_OPT_PIPE_CHAIN): lane l's epoch
  // `seq` numbered and appended on the device right after its decision, from
  // this context's device tnc / append position (fin_ctl), which the finish
  // advances; `after`: the previous epoch's last work (its finish) is waited
  // for on the device; reset: fin_ctl starts at this context's values
  int chain_enqueue(dcc_ctx* l, uint64_t seq, hipEvent_t after, bool reset);
  // fin_ctl = {tnc, delta size, seq} after lane l's work: the host finished
  // the epoch before `seq` itself
  int chain_set(dcc_ctx* l, uint64_t seq);
  // the chained finish of lane l's epoch numbered it: tnc and the delta level follow
  int chain_accept(dcc_ctx* l);
  uint64_t hist_room() const;  // flat pairs the delta level holds without moving
  DevBuf fin_ctl;                  // parent: dcc::FinCtl
  DevBuf fdyn;                     // lane: the chained finish's OccDyn
  void* hfin = nullptr;            // lane: its staging and totals (pinned, HDYN_BYTES)
  void* hfin_dev = nullptr;
  hipEvent_t ev_done = nullptr;    // lane: after the work of its last submitted epoch
  uint32_t pipe_chain = 1;         // DCC_OPT_PIPE_CHAIN
  int occ_end(dcc_stats* st);
  int occ_final(bool async);  // finalize launches (or the graph replay) of `run`
  // pipelined epochs over lane contexts on this device (occ_pipe.cpp)
  struct OccPipe* pipe = nullptr;
  uint32_t pipe_lanes = 3;  // DCC_OPT_PIPELINE
  uint32_t pipe_part = 0;   // DCC_OPT_PIPE_PARTITION
  int cv_path = 0;          // DCC_OPT_CALVIN_PATH: 0 auto, 1 sort, 2 bucket
  bool cb_hash_off = false; // a hashed bucket carry table overflowed: sort path for such epochs
  // DCC_OCC_DEFER_FINISH: the decided epoch waiting for its global RC
  bool fin_pending = false;
  DevBatch fin_d;
  uint64_t fin_nnz_w = 0;
  DevBuf fin_off, fin_keys, fin_at, fin_state, fin_hasw, fin_rc, fin_cnt;
  int fin_save(const DevBatch& d, bool host_batch, uint64_t nnz_w);
  int occ_finish(const uint8_t* final_rc, uint64_t* out_tn, uint32_t flags);
  int occ_finish_prepare(const uint8_t* final_rc, uint32_t flags, uint32_t& n_cw);
  int occ_finish_commit(uint32_t n_cw, uint64_t* out_tn, uint32_t flags);
  int occ_rounds(const SubProb& sp, uint32_t maxlen, bool prof, uint32_t& rounds);
  int sweep_reserve(const DevBatch& d);
  // levels [l0, l1); resume: level l0's serial part already ran (start at its
  // committed-set listing); tail_serial: level l1 - 1 runs its serial part only
  int sweep_enqueue(const DevBatch& d, int l0, int l1, const dcc::SwShard* shard = nullptr,
                    bool resume = false, bool tail_serial = false);
  int sweep_sharded(const DevBatch& d, int& next_level);
  int sweep_sharded_full(const DevBatch& d, const DevBatch& full, int l0, int l1);  // levels [l0, l1)
  // decide the RO list (full: a key-sharded rank's whole batch)
  int sweep_ro(const DevBatch& d, bool big, bool scan, uint64_t nnz_w, const DevBatch* full = nullptr);
  int occ_sweep_finish(const DevBatch& d, int& next_level, bool& done, uint32_t maxlen);
  int occ_snapshot(const dcc_batch* b, const dcc_occ_snapshot* s, uint8_t* out_rc, dcc_stats* st);
  // MaaT (maat.hip): epoch workspaces
  int index_reserve(uint64_t want);
  int maat_epoch(const dcc_batch* b, uint8_t* out_rc, uint64_t* out_cts, dcc_stats* st);
  int maat_epoch_try(const dcc_batch* b, uint8_t* out_rc, uint64_t* out_cts, dcc_stats* st, bool all_rows,
                     bool* full);
  int calvin_epoch(const dcc_batch* b, const dcc_calvin_held* held, uint32_t* out_group,
                   uint8_t* out_rc, uint32_t* out_wave, dcc_stats* st);
  // NO_WAIT 2PL (nowait.hip)
  // whole_table: room in `table` for every request (a key-sharded epoch sizes its own)
  int nowait_reserve(uint64_t n, uint64_t nnz, bool with_conflict, bool whole_table = true);
  // lt: the epoch runs against this lock table and leaves its grants in it
  int nowait_epoch(const dcc_batch* b, const dcc_calvin_held* held, uint8_t* out_rc,
                   uint32_t* out_conflict, dcc_stats* st, dcc_locktab* lt = nullptr);
  // lock table (locktab.hip): the calls on the context that runs them.  An
  // epoch calls begin (room for `incoming` requests, rebuilding if needed;
  // control words cleared), seed after the per-epoch table is built, grant
  // after the decisions (it enqueues the read-back too) and, after the
  // epoch's last synchronisation found no error, end (the host state follows)
  static constexpr size_t LT_HMISC_OFF = 1024;  // the table's control words in hmisc
  int locktab_alloc(dcc_locktab* lt);
  int locktab_begin(dcc_locktab* lt, uint64_t incoming, const char* what);
  int locktab_seed(dcc_locktab* lt, const LtEpoch& E);
  int locktab_grant(dcc_locktab* lt, const LtEpoch& E);
  int locktab_end(dcc_locktab* lt, uint64_t* granted);
  int locktab_release(dcc_locktab* lt, const dcc_batch* b, const uint8_t* rc_in, uint8_t want,
                      const uint64_t* keys, uint64_t n_keys, bool keys_dev, uint64_t* out_n,
                      uint64_t* out_nnz, dcc_stats* st);
  int locktab_acquire(dcc_locktab* lt, const dcc_calvin_held* rows, bool dev);
  int locktab_export(dcc_locktab* lt, uint64_t* keys, uint8_t* lock_type, uint32_t* owner_cnt,
                     uint64_t cap, bool dev, uint64_t* out_n);
  int locktab_clear(dcc_locktab* lt);
  // select by decision into a CSR (select.hip)
  int select_reserve(uint64_t n, uint64_t nnz);
  int select_batch(const dcc_batch* b, const uint8_t* rc_in, uint8_t want, const uint32_t* src_in,
                   const dcc_select_out* out, uint64_t* out_n, uint64_t* out_nnz, dcc_stats* st);
  // abort queue (abortq.hip): the calls on the context that runs them
  int abortq_alloc(dcc_abortq* q);
  int abortq_push(dcc_abortq* q, const dcc_batch* b, const uint8_t* rc_in, uint8_t want, const uint32_t* src_in,
                  const uint32_t* cnt_in, uint64_t now, uint64_t* out_n, uint64_t* out_nnz, dcc_stats* st);
  int abortq_pop(dcc_abortq* q, uint64_t now, const dcc_select_out* out, uint32_t* out_cnt, uint64_t* out_due,
                 uint32_t flags, uint64_t* out_n, uint64_t* out_nnz, dcc_stats* st);
  // device-side key-shard partition (shard_dev.hip): rank `rank` of R of a
  // multi-GPU context; sb is the shard as a device batch
  DevBuf sh_off, sh_keys, sh_at, sh_src, sh_cnt, sh_bsum, sh_rc, sh_tn, sh_grp;
  int shard_stage(const dcc_batch* b, uint32_t rank, uint32_t R, dcc_batch& sb, DevBatch* full_out = nullptr);
  int shard_groups(const uint32_t* grp, uint64_t m, uint32_t* out_dev);  // groups to batch order
  // lock tables created on this context and not yet destroyed (freed with it)
  std::vector<std::unique_ptr<dcc_locktab>> locktabs;
  // the sorted-segment epochs' workspaces (TIMESTAMP, MVCC, WAIT_DIE)
  SegWork seg;
  // TIMESTAMP epoch (tso.hip): the persistent row table {key, wts, rts}; head
  // slots, bounds, the timestamps and conflict ordinals of a host call
  RowTab ts_rows{"tso"};
  DevBuf ts_hslot, ts_bnd, ts_stage, ts_conf;
  int tso_reserve(uint64_t n, uint64_t nnz, bool with_conflict);
  int tso_epoch(const dcc_batch* b, const uint64_t* ts, uint8_t* out_rc, uint32_t* out_conflict,
                dcc_stats* st);
  // MVCC epoch (mvcc.hip): the persistent row table {key, latest version,
  // rts}; the version store, (key, ts) pairs sorted by (key, ts) in buffer
  // mv_cur of two (a merge or a trim writes the other one and swaps); the
  // epoch's versions (key, ts, txn), the late accesses, the rows' slots at the
  // segment ends, tile offsets, the versions out of a host call.  The
  // decisions run in `seg` and the TIMESTAMP epoch's workspaces.
  RowTab mv_rows{"mvcc"};
  DevBuf mv_sk[2], mv_st[2];
  int mv_cur = 0;
  uint64_t mv_n = 0;  // versions in the store
  DevBuf mv_ek, mv_et, mv_ex, mv_late, mv_lslot, mv_toff, mv_vts;
  int mvcc_reserve(uint64_t n, uint64_t nnz, bool with_conflict, bool with_vts);
  int mvcc_store_room(uint64_t need);
  int mvcc_epoch(const dcc_batch* b, const uint64_t* ts, uint8_t* out_rc, uint32_t* out_conflict,
                 uint64_t* out_vts, dcc_stats* st);
  int mvcc_trim(uint64_t floor, uint64_t* n_dropped);
  int mvcc_export(uint64_t* keys, uint64_t* ts, uint64_t cap, uint64_t* n_out);
  // the live-txn calls' workspaces next to `seg` (live_txn.h): flag bytes, a host call's state and conflicts
  DevBuf lv_flg;
  DevBuf lv_hts, lv_hrc, lv_hpos, lv_hleave, lv_conf;
  int live_reserve(uint64_t n, uint64_t nnz, bool host_arrays);
  int live_stage(uint64_t n, bool dev, const uint64_t* ts, uint8_t* rc, uint32_t* pos, const uint8_t* leave,
                 const uint64_t*& ts_d, uint8_t*& rc_d, uint32_t*& pos_d, const uint8_t*& leave_d);
  // WAIT_DIE (waitdie.hip).  The lock state is the caller's (rc, pos) arrays
  int waitdie_epoch(const dcc_batch* b, const uint64_t* ts, uint8_t* rc, uint32_t* pos, uint32_t* out_conflict,
                    dcc_stats* st);
  int waitdie_release(const dcc_batch* b, const uint64_t* ts, uint8_t* rc, uint32_t* pos, const uint8_t* leave,
                      uint64_t* out_left, uint64_t* out_promoted, dcc_stats* st);
  // the population's carry between two epochs (waitdie_carry.hip).  Control
  // words and tile pairs are the select's; of a host call the population's
  // state goes through the staging above (revive through lv_hleave, src_in
  // through sel_src), the fresh batch and the outputs through these
  DevBuf wc_foff, wc_fkeys, wc_fat, wc_fts, wc_out;
  int carry_reserve(uint64_t n, uint64_t nnz);
  int waitdie_carry(const dcc_waitdie_carry_args* a, uint64_t* out_n, uint64_t* out_nnz, uint64_t* out_kept,
                    dcc_stats* st);
  // key-sharded NO_WAIT epoch (nowait.hip): a status byte per txn (the rounds'
  // exchange, then 64 - the conflict ordinal); a multi-GPU context's per-rank
  // conflict ordinals of a device batch
  DevBuf nw_stat, sh_conf;
  // MVCC with txns in flight (mvcc_live.hip).  The state is the caller's (rc,
  // pos) arrays, rows and versions are the MVCC epoch's above; the workspaces
  // are the live-txn calls', the TIMESTAMP epoch's head slots and the MVCC
  // epoch's version lists
  int mvcc_live_reserve(uint64_t n, uint64_t nnz, bool host_arrays);
  int mvcc_access_epoch(const dcc_batch* b, const uint64_t* ts, uint8_t* rc, uint32_t* pos, uint64_t* vts,
                        uint32_t* out_conflict, dcc_stats* st);
  int mvcc_finish(const dcc_batch* b, const uint64_t* ts, uint8_t* rc, uint32_t* pos, const uint8_t* leave,
                  uint64_t* vts, uint64_t* out_left, uint64_t* out_promoted, dcc_stats* st);
  // TIMESTAMP with txns in flight (tso_live.hip).  The state is the caller's
  // (rc, pos) arrays, the rows are the TIMESTAMP epoch's ts_rows above; the
  // workspaces are the live-txn calls' and the TIMESTAMP epoch's head slots
  int tso_live_reserve(uint64_t n, uint64_t nnz, bool host_arrays);
  int tso_access_epoch(const dcc_batch* b, const uint64_t* ts, uint8_t* rc, uint32_t* pos, uint32_t* out_conflict,
                       dcc_stats* st);
  int tso_finish(const dcc_batch* b, const uint64_t* ts, uint8_t* rc, uint32_t* pos, const uint8_t* leave,
                 uint64_t* out_left, uint64_t* out_promoted, dcc_stats* st);
};

// The host-side return-on-failure frame: CK takes a HIP call (the message goes
// to `ctx`, a dcc_ctx* in scope), CR a call that returns a DCC code.
#define CK(expr)                                           \
  do {                                                     \
    hipError_t e_ = (expr);                                \
    if (e_ != hipSuccess) return ctx->hip_fail(e_, #expr); \
  } while (0)
#define CR(expr)                 \
  do {                           \
    int r_ = (expr);             \
    if (r_ != DCC_OK) return r_; \
  } while (0)

// The stats of a single-GPU epoch: constructed first thing (the wall clock
// starts, S is zeroed with one shard), finished after the epoch's last
// synchronisation.
struct EpochStats {
  dcc_stats S;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  EpochStats() {
    memset(&S, 0, sizeof S);
    S.n_shards = 1;
  }
  void wall() {
    S.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  // device_ms from ev0 / ev1, phase_ms[0, phases) from pev when profiling, total_ms
  int finish(dcc_ctx* ctx, int phases) {
    float ms = 0;
    CK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    S.device_ms = ms;
    for (int q = 0; ctx->profiling && q < phases; q++) {
      CK(hipEventElapsedTime(&ms, ctx->pev[q], ctx->pev[q + 1]));
      S.phase_ms[q] = ms;
    }
    wall();
    return DCC_OK;
  }
};

// Workgroups for `items` at `per_block` each: at least one, at most max_grid
// (the kernels stride).
inline unsigned launch_grid(uint64_t items, uint64_t per_block, unsigned max_grid) {
  const uint64_t b = (items + per_block - 1) / per_block;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(b, max_grid));
}

// multi-GPU context (dcc_multi.cpp)
int dcc_multi_size(const dcc_ctx* ctx);
void dcc_multi_destroy(dcc_ctx* ctx);
int dcc_multi_occ_epoch(dcc_ctx* ctx, const dcc_batch* b, uint8_t* out_rc, uint64_t* out_tn,
                        dcc_stats* st);
int dcc_multi_calvin_epoch(dcc_ctx* ctx, const dcc_batch* b, const dcc_calvin_held* held,
                           uint32_t* out_group, uint8_t* out_rc, uint32_t* out_wave, dcc_stats* st);
int dcc_multi_nowait_epoch(dcc_ctx* ctx, const dcc_batch* b, const dcc_calvin_held* held, uint8_t* out_rc,
                           uint32_t* out_conflict, dcc_stats* st);
int dcc_multi_each(dcc_ctx* ctx, int (*fn)(dcc_ctx*, void*), void* user);
int dcc_multi_occ_snapshot(dcc_ctx* ctx, const dcc_batch* b, const dcc_occ_snapshot* snap,
                           uint8_t* out_rc, dcc_stats* st);
dcc_ctx* dcc_multi_rank0(dcc_ctx* ctx);  // rank 0's sub-context, its device selected
// pipelined epochs (occ_pipe.cpp): complete every epoch in flight / tear down
void dcc_pipe_drain(dcc_ctx* ctx);
void dcc_pipe_destroy(dcc_ctx* ctx);
dcc_ctx* dcc_multi_sub(dcc_ctx* ctx, int rank);

// A single-GPU engine's call on a multi-GPU context: run on rank 0's
// sub-context with its device selected -- `detach`: without its communicator,
// so that the engine makes no collective -- and the failure text copied up.
template <typename F>
int dcc_multi_on_rank0(dcc_ctx* ctx, bool detach, F call) {
  dcc_ctx* s = dcc_multi_rank0(ctx);
  dcc_comm_state* const cm = s->comm;
  if (detach) s->comm = nullptr;
  const int e = call(s);
  s->comm = cm;
  if (e != DCC_OK) ctx->last_error = s->last_error;
  return e;
}
// The same for any context: a one-GPU context runs the call itself, its
// device selected.
template <typename F>
int dcc_on_device(dcc_ctx* ctx, bool detach, F call) {
  if (ctx->multi) return dcc_multi_on_rank0(ctx, detach, call);
  if (hipSetDevice(ctx->device) != hipSuccess) return DCC_ENODEV;
  return call(ctx);
}
