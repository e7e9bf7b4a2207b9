/*
 * dcc.h — C ABI of the MI355X-native batched concurrency-control engine
 * (libdcc.so).  Everything a Deneva-style host binds to for the one hot path
 * SURVEY.md §8 scopes: deciding commit/abort (OCC) and lock-grant order
 * (Calvin) for a whole epoch of transactions at once.
 *
 * Conventions:
 *   - extern "C", plain pointers and sizes, no torch / HIP types in signatures
 *     (streams are passed as opaque `void*`).
 *   - every entry point returns int: 0 = success, < 0 = -errno-style code
 *     (DCC_E*).  Nothing aborts the process; batch validation (offset
 *     monotonicity, nnz bound, reserved key) runs on the host before launch.
 *   - all pointers are caller-owned; nothing is retained after return.
 *   - a dcc_ctx is thread-compatible, not thread-safe: the host shim
 *     serialises calls per context (reference OptCC serialises its list
 *     mutations with `_semaphore`, concurrency_control/occ.cpp:137-158).
 *
 * Reference interfaces each entry point replaces are cited per declaration
 * (paths relative to the reference tree).
 */
#ifndef DCC_H_
#define DCC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- errors */
#define DCC_OK 0
#define DCC_EIO (-5)       /* HIP runtime failure (message via dcc_last_error) */
#define DCC_ENOMEM (-12)   /* device or host allocation failed                  */
#define DCC_ENODEV (-19)   /* no usable gfx950 device / bad device id           */
#define DCC_EINVAL (-22)   /* malformed batch or argument                       */
#define DCC_ERANGE (-34)   /* size exceeds an engine limit                      */
#define DCC_ECOMM (-70)    /* RCCL failure                                       */
#define DCC_ENOTSUP (-95)  /* feature not available in this build / mode        */

/* ------------------------------------------------------ reference enums */
/* access_t, system/global.h:287  {RD, WR, XP, SCAN}.  OCC puts only WR into
 * the write set (concurrency_control/occ.cpp:296-317, get_rw_set: `get_access_type(i) == WR`, line 308); Calvin
 * maps RD/SCAN to LOCK_SH and everything else to LOCK_EX (storage/row.cpp:191). */
#define DCC_RD 0
#define DCC_WR 1
#define DCC_XP 2
#define DCC_SCAN 3

/* RC, system/global.h:236  {RCOK=0, Commit, Abort, WAIT, ...}.  The engine
 * reports per-transaction RCs with the reference's numeric values. */
#define DCC_RC_RCOK 0
#define DCC_RC_ABORT 2
#define DCC_RC_WAIT 3

/* Keys are canonical 64-bit row identities.  This
 * one value is reserved as the empty-slot marker of the device hash table. */
#define DCC_KEY_RESERVED 0xFFFFFFFFFFFFFFFFull

/* group value for a Calvin request removed by per-txn row de-duplication
 * (TxnManager::get_lock, system/txn.cpp:778-782). */
#define DCC_GROUP_NONE 0xFFFFFFFFu

/* --------------------------------------------------------------- batch  */
/* dcc_batch.flags */
#define DCC_DEVICE_PTRS 0x1u      /* every batch AND output pointer is device memory */
#define DCC_MAAT_READ_AND_PREWRITE 0x4u /* MaaT: every access both reads and prewrites its row
                                          (the TPC-C path, Row_maat::read_and_prewrite,
                                          row_maat.cpp:40-41, 54-96)                     */
#define DCC_OCC_APPEND_HISTORY 0x2u /* central_finish semantics: committed write sets
                                     of this epoch are appended to the history with
                                     tn = tnc+1, tnc+2, ... in index order
                                     (occ.cpp:248-294) */
#define DCC_OCC_DEFER_FINISH 0x8u   /* 2PC participants: decide only.  Commit tn and the
                                     history follow the GLOBAL RC passed later to
                                     dcc_occ_finish_epoch (OptCC::finish after RFIN,
                                     worker_thread.cpp:286-297, occ.cpp:248-294).  Not
                                     with DCC_OCC_APPEND_HISTORY or out_commit_tn. */

/* Compact transfer forms (host or device batches; widened on the device before
 * any kernel reads them).  They shrink what a host batch moves over PCIe:
 * u32 keys halve the largest array when the key universe fits (YCSB row ids),
 * packed access types and u32 timestamps cut the rest. */
#define DCC_KEYS_U32 0x10u      /* keys points to uint32_t keys                            */
#define DCC_ACCTYPE_2BIT 0x20u  /* acctype holds 2-bit access types, four per byte: access x
                                   in bits 2(x%4)..2(x%4)+1 of byte x/4                     */
#define DCC_TN_U32 0x40u        /* start_tn / finish_tn point to uint32_t timestamps        */
#define DCC_COMPACT_FLAGS (DCC_KEYS_U32 | DCC_ACCTYPE_2BIT | DCC_TN_U32)
/* Key-sharded contexts (dcc_comm_init*): the batch is the WHOLE epoch; the
 * rank keeps its key shard of the accesses itself (partitioned on the device)
 * and the whole batch for the serial passes, so ranks exchange only kill bits
 * (one fixed-size all-gather per sweep level, no host synchronisation between
 * levels).  Without the flag a rank passes only its own accesses
 * (dcc_shard_filter) and the ranks exchange the serial ranges' records.
 * A multi-GPU context (dcc_init_multi) always shards this way.
 * dcc_nowait_lock_epoch takes the flag too (its comment has the contract):
 * without it that call is not key-sharded at all.  On a context that is not
 * key-sharded the flag is ignored. */
#define DCC_SHARD_SELF 0x80u
/* ISOLATION_LEVEL of a 2PL NO_WAIT epoch (config.h; ycsb_txn.cpp:233-236,
 * 248-251, txn.cpp:692-726).  Neither bit: SERIALIZABLE.  Both: DCC_EINVAL.
 * The level is a property of the epoch, not of a context or a lock table.
 * dcc_nowait_lock_epoch, dcc_locktab_lock_epoch and dcc_locktab_release honour
 * the bits (their comments have the contract); dcc_waitdie_lock_epoch,
 * dcc_waitdie_release and dcc_waitdie_carry are DCC_ENOTSUP with one set (a
 * read released inside a WAIT_DIE epoch would promote waiters mid-epoch).
 * Every other entry point ignores them: OCC, TIMESTAMP, MVCC, MaaT and Calvin
 * are not modelled below SERIALIZABLE. */
#define DCC_ISO_READ_COMMITTED 0x100u   /* a read lock is released right after the read   */
#define DCC_ISO_READ_UNCOMMITTED 0x200u /* every lock is released right after its access  */

/* One epoch as a CSR of per-transaction access lists in capture order
 * (Access list of TxnManager, system/txn.h:39-70; txn.cpp:818-847). */
typedef struct dcc_batch {
  uint64_t n_txn;
  uint64_t nnz;
  const uint32_t* offsets;   /* [n_txn+1]; offsets[0]=0, non-decreasing, offsets[n_txn]=nnz */
  const uint64_t* keys;      /* [nnz] canonical keys, != DCC_KEY_RESERVED                */
  const uint8_t* acctype;    /* [nnz] access_t                                           */
  const uint64_t* start_tn;  /* [n_txn] txn start ts (worker_thread.cpp:500-502) or NULL */
  const uint64_t* finish_tn; /* [n_txn] validation ts (occ.cpp:142) or NULL.  Both NULL
                                disables the history window check, which is exactly
                                the reference behaviour under TS_CLOCK */
  const uint64_t* order;     /* Calvin: [n_txn] sequence key (epoch<<48|origin<<32|seq,
                                any monotone encoding) or NULL = index order             */
  uint32_t flags;
  uint32_t reserved;
} dcc_batch;

typedef struct dcc_stats {
  uint32_t rounds;       /* fixed-point rounds executed                                */
  uint32_t n_shards;     /* GPUs that took part                                        */
  uint64_t n_commit;     /* RCOK decisions (Calvin: ready at acquire)                  */
  uint64_t n_abort;      /* Abort decisions (Calvin: WAIT)                             */
  uint64_t n_readonly;   /* txns with an empty write set                               */
  uint64_t nnz_w;        /* write accesses                                             */
  uint64_t alg_bytes;    /* algorithmic bytes of one pass, SURVEY.md §8(d)             */
  double device_ms;      /* device time of the decision, batch resident                */
  double total_ms;       /* wall time of the call incl. H2D/D2H when host pointers      */
  /* Per-phase device time (HIP events on the engine stream; filled only when
   * profiling is enabled with dcc_set_profiling) and the algorithmic bytes
   * of each phase.  OCC sweep: 0 = level-0 tile records + serial pass,
   * 1 = level-0 filter, 2 = later levels (and any round-solver hand-off),
   * 3 = prep + finalize; round solver only: 0 = key-hash build, 1 = round 1,
   * 2 = rounds >= 2, 3 = prep + finalize.  Calvin: 0 = build, 1 = grant
   * groups, 2 = waves, 3 = prep + finalize. */
  double phase_ms[4];
  uint64_t phase_bytes[4];
  /* OCC sweep: the level-0 serial prefix (0 = the epoch was
   * decided by rounds alone) and the txns that survived the level-0 filter.
   * The sweep reports its levels in `rounds`. */
  uint64_t peel_prefix;
  uint64_t n_survivors;
  uint32_t fallback;     /* sweep lists handed to the round solver (they stopped
                            shrinking); the decisions are the same                    */
  uint32_t fin_where;    /* pipelined epochs with commit tn / append (dcc_occ_wait_epoch):
                            1 numbered on the device behind the decision (chained),
                            2 by the context at completion; 0 otherwise              */
} dcc_stats;

/* ------------------------------------------------------------- context  */
typedef struct dcc_ctx dcc_ctx;

/* Replaces OptCC::init (occ.cpp:33-40) and the global occ_man singleton
 * (system/global.cpp:42): one context per process and device.
 * device_id < 0 selects the current HIP device. */
int dcc_init(dcc_ctx** out, int device_id);
/* One process, n GPUs (multi-GPU internal to the context):
 * the context key-shards every epoch over n per-device sub-contexts
 * (dcc_key_shard) that exchange over one RCCL clique (ncclCommInitAll) when
 * the ids are distinct, else over an in-process host exchange (shards sharing
 * a GPU).  Each sub-context partitions the batch on its own GPU (a host batch
 * is copied to every GPU; a device batch, DCC_DEVICE_PTRS, is read where it
 * lies -- peer access between distinct GPUs is enabled here).  OCC and Calvin
 * epochs return the same decisions as one GPU (device outputs are written by
 * rank 0); options, tnc and history apply to every shard.  Captured-snapshot
 * validation is key-sharded too (each rank against its history shard; a txn
 * commits iff every rank commits it).  Calvin wave levels and MaaT run the
 * whole epoch on rank 0's GPU (the levels chain through every row; MaaT's
 * bounds combine every row of a txn; its row table lives on rank 0).
 * dcc_set_stream is DCC_ENOTSUP on it. */
int dcc_init_multi(dcc_ctx** out, int n_gpus, const int* device_ids);
void dcc_destroy(dcc_ctx* ctx);
const char* dcc_strerror(int code);
const char* dcc_last_error(const dcc_ctx* ctx); /* detail of the last failure */
int dcc_version(void);                            /* 100*major + minor */
int dcc_device_count(void);                       /* gfx950 devices visible (0 if none) */

/* Run on an external HIP stream (opaque hipStream_t, e.g. torch's current
 * stream).  NULL restores the context's own stream. */
int dcc_set_stream(dcc_ctx* ctx, void* hip_stream);
/* Record per-phase HIP events inside every call (dcc_stats.phase_ms). */
int dcc_set_profiling(dcc_ctx* ctx, int enable);
/* Tuning knobs (defaults are the tuned values; for A/B measurement). */
#define DCC_OPT_RECHECK 1     /* fold kill waves into rounds whose list has <= value txns */
#define DCC_OPT_BATCH_MAX 2   /* max rounds enqueued between host synchronisations        */
#define DCC_OPT_SOLVER 5      /* OCC solver: 0 auto (= 3), 1 fixed-point rounds only, 3 sweep
                                 (levels of serial passes + filters; hands lists that stop
                                 shrinking to the round solver)                              */
#define DCC_OPT_SWEEP_LEVELS 6 /* sweep levels enqueued between host synchronisations (0:
                                  auto, 3 with DCC_OPT_RO_SPLIT, 4 without)                  */
#define DCC_OPT_HIST_MERGE 7  /* device history: delta pairs above which the delta merges into
                                 the base (default 65536; the base/4 rule also applies)      */
#define DCC_OPT_RO_SPLIT 10   /* sweep: read-only txns that survive the first level's filter
                                 leave the level lists and are decided once every writer is
                                 (1, default) or stay in the lists (0); one-GPU epochs only.
                                 4..24: on, with 2^value committed-writer table slots (the
                                 table grows after an overflow; tests use small ones)        */
#define DCC_OPT_FAIL_RANK 8   /* fault injection (tests): rank `value` of a multi-GPU context
                                 fails its next epoch before its first exchange; the other
                                 ranks must return DCC_ECOMM instead of waiting for it      */
#define DCC_OPT_PIPELINE 11   /* lanes of dcc_occ_submit_epoch: epochs in flight at once
                                 (1..8, default 3).  Each lane is a HIP stream that needs a
                                 hardware queue of its own: run with GPU_MAX_HW_QUEUES >=
                                 lanes + the caller's streams (HIP's default of 4 makes
                                 lanes share queues, which serialises them)                 */
#define DCC_OPT_CALVIN_PATH 12 /* Calvin grant groups: 0 auto (the bucket path for epochs of
                                  >= 2M requests it applies to), 1 the global key sort + scan,
                                  2 the bucket path wherever it applies                       */
#define DCC_OPT_COMM_SOLO 13  /* tests: with 1, a later dcc_comm_init(ctx, 0, 1, id) forms a
                                 one-rank RCCL clique and the context runs the key-sharded
                                 paths with their collectives (ncclAllReduce / ncclAllGather
                                 over the one rank) instead of the one-GPU paths: the RCCL
                                 call path executes on a one-GPU box                         */
#define DCC_OPT_PIPE_PARTITION 14 /* pipeline lanes on their own CUs: 0 every lane on the whole
                                  chip; 1 lane i of L on 1/L of the CUs of every XCD (its
                                  stream CU-masked), so a lane's serial passes never queue
                                  behind another lane's chip-wide kernels (L must divide
                                  n_CU / 8; otherwise the lanes stay unmasked)             */
#define DCC_OPT_PIPE_CHAIN 15 /* pipelined epochs with commit tn / history append: 1 (default)
                                 each lane numbers and appends its epoch on the device right
                                 after deciding it, from a device copy of tnc and the append
                                 position that the epochs advance in submit order; 0 the
                                 context finishes each epoch on its lane's completion     */
int dcc_set_option(dcc_ctx* ctx, int option, int64_t value);
/* Pre-size device workspaces so a later call performs no allocation. */
int dcc_reserve(dcc_ctx* ctx, uint64_t max_txn, uint64_t max_nnz);
/* Achievable HBM bandwidth on this device (measurement aid):
 * hand-written 16-byte-per-lane copy kernels over two `bytes`-sized device
 * buffers (grid-stride; one contiguous range per workgroup with non-temporal
 * loads and stores at 2 / 4 / 8 workgroups per CU), `reps` launches of each
 * timed with HIP events; *gbps = 2 * bytes / time of the fastest form. */
int dcc_copy_bandwidth(dcc_ctx* ctx, uint64_t bytes, int reps, double* gbps);
/* Pinned (page-locked) host memory for batches and outputs: a host batch in it
 * is copied at DMA speed with no staging copy.  Free with dcc_host_free. */
int dcc_host_alloc(dcc_ctx* ctx, uint64_t bytes, void** out);
int dcc_host_free(dcc_ctx* ctx, void* p);  /* ctx may be NULL */

/* ------------------------------------------------------- multi-GPU     */
/* Key sharding across the GPUs of one node, one process per GPU
 * (SURVEY.md §8(e)).  Each rank owns keys with dcc_key_shard(key, n) == rank,
 * receives the full per-txn offsets plus only its own accesses, and joins a
 * per-round RCCL ncclMax allreduce of per-txn state bytes — the MI355X form
 * of 2PC's AND of per-node OK bits (worker_thread.cpp:328-334). */
#define DCC_UNIQUE_ID_BYTES 128
int dcc_comm_unique_id(void* out_id /* DCC_UNIQUE_ID_BYTES */);
/* RCCL communicator: every rank passes rank 0's unique id. */
int dcc_comm_init(dcc_ctx* ctx, int rank, int nranks, const void* unique_id);
/* Host-exchange communicator: `fn` all-reduces n bytes in place with MAX
 * across the ranks (returns 0 on success).  For harnesses whose ranks cannot
 * form an RCCL clique, e.g. several ranks sharing one GPU in tests. */
typedef int (*dcc_exchange_fn)(void* user, uint8_t* host_buf, uint64_t n);
int dcc_comm_init_host(dcc_ctx* ctx, int rank, int nranks, dcc_exchange_fn fn, void* user);
int dcc_comm_destroy(dcc_ctx* ctx);
int dcc_comm_rank(const dcc_ctx* ctx);
int dcc_comm_size(const dcc_ctx* ctx);
/* Collectives this context's communicator has run since dcc_comm_init (RCCL
 * calls enqueued, or host exchanges); 0 without a communicator. */
uint64_t dcc_comm_calls(const dcc_ctx* ctx);
uint32_t dcc_key_shard(uint64_t key, uint32_t nranks);
/* dcc_key_shard of n keys (host arrays): out[i] = shard of keys[i] */
int dcc_key_shard_n(const uint64_t* keys, uint64_t n, uint32_t nranks, uint32_t* out);
/* Host helper: keep only the accesses of `rank` (same n_txn, same order).
 * out_offsets [n_txn+1]; out_keys/out_acctype sized >= in nnz; *out_nnz set. */
int dcc_shard_filter(const dcc_batch* in, uint32_t rank, uint32_t nranks,
                     uint32_t* out_offsets, uint64_t* out_keys,
                     uint8_t* out_acctype, uint64_t* out_nnz);

/* ------------------------------------------------------------------ OCC */
/* Epoch validation: the result equals validating every txn of the batch in
 * index order with OptCC::central_validate (occ.cpp:116-239) and only then
 * finishing all of them with central_finish (occ.cpp:248-294).
 *   out_rc[i]        = DCC_RC_RCOK or DCC_RC_ABORT (TxnManager::validate, txn.cpp:935)
 *   out_commit_tn[i] = history tn given to committed non-read-only txns, else 0
 *                      (tnc++ / wset->tn = tnc, occ.cpp:283-284); may be NULL. */
int dcc_occ_validate_epoch(dcc_ctx* ctx, const dcc_batch* batch, uint8_t* out_rc,
                           uint64_t* out_commit_tn, dcc_stats* out_stats);
/* (Any entry point: when a call returns an error, the contents of its output
 * arrays are unspecified -- e.g. a malformed host batch, whose offsets the
 * device checks, may already have been decided into out_rc.) */
/* Pipelined epochs (one GPU).  dcc_occ_submit_epoch enqueues an epoch and
 * returns without waiting for it.  Consecutive epochs run on separate lanes
 * (DCC_OPT_PIPELINE of them, each with its own stream, workspaces and
 * captured graph), so one epoch's latency-bound serial passes overlap the
 * next epoch's streaming passes.  The results are exactly those of calling
 * dcc_occ_validate_epoch on the epochs in submit order: under TS_CLOCK (no
 * history window) epochs of central_validate are
 * independent except for central_finish's commit counter and history
 * (occ.cpp:277-286), so each lane decides its epoch and its central_finish --
 * commit tn (out_commit_tn) and the DCC_OCC_APPEND_HISTORY append -- runs in
 * submit order: on the device right after the decision, once the epoch before
 * it has finished (DCC_OPT_PIPE_CHAIN), or by the context when the epoch
 * completes.  An epoch that fails after its finish ran on the device fails
 * the epochs in flight behind it too (their numbering followed it).  An epoch that needs the epochs before it finished -- a window
 * against a non-empty history or against appends still in flight,
 * DCC_OCC_DEFER_FINISH -- or profiling, the round solver, or a multi-GPU or
 * key-sharded context first drains the pipeline and then runs
 * synchronously, still in submit order.  The batch arrays and the outputs
 * must stay valid and unchanged until the epoch's dcc_occ_wait_epoch
 * returns.  *out_ticket (1, 2, ...) names the epoch.  Argument errors are
 * returned by submit; the epoch's own result by wait.
 * dcc_occ_wait_epoch completes, in submit order, every epoch up to `ticket`
 * and returns that epoch's status and stats.  Each ticket is waited once;
 * earlier tickets keep their results until they are waited.  Every other
 * OCC entry point on the context (validate, finish, history, tnc) first
 * completes the epochs in flight. */
int dcc_occ_submit_epoch(dcc_ctx* ctx, const dcc_batch* batch, uint8_t* out_rc,
                         uint64_t* out_commit_tn, uint64_t* out_ticket);
int dcc_occ_wait_epoch(dcc_ctx* ctx, uint64_t ticket, dcc_stats* out_stats);
/* central_finish with the global decision, for an epoch validated with
 * DCC_OCC_DEFER_FINISH (each node votes with its local RC; 2PC's coordinator
 * commits only if every participant voted RCOK, worker_thread.cpp:328-334,
 * and RFIN carries that RC back, worker_thread.cpp:286-297):
 *   final_rc[i] = DCC_RC_RCOK or DCC_RC_ABORT, the global RC of txn i;
 * committed non-read-only txns (global RCOK) take tn = tnc+1, tnc+2, ... in
 * index order and their write sets join the history; a txn aborted globally
 * leaves no trace even if it validated locally.  DCC_EINVAL if a txn has
 * final RCOK but aborted locally (2PC never commits it) or no epoch is
 * pending.  flags: DCC_DEVICE_PTRS when final_rc / out_commit_tn are device
 * memory.  The deferred epoch's device batch (DCC_DEVICE_PTRS) must stay
 * valid until this call; every other OCC epoch is refused meanwhile. */
int dcc_occ_finish_epoch(dcc_ctx* ctx, const uint8_t* final_rc, uint64_t* out_commit_tn,
                         uint32_t flags);
/* Committed write sets of earlier epochs (the `history` list, occ.h:62-64).
 * keys/tn are host arrays of n (key, tn) pairs; each pair is one write of the
 * committed txn numbered tn.  The history is device-resident: epochs with
 * DCC_OCC_APPEND_HISTORY append their committed writes on the device. */
int dcc_occ_history_append(dcc_ctx* ctx, const uint64_t* keys, const uint64_t* tn, uint64_t n);
int dcc_occ_history_clear(dcc_ctx* ctx);
uint64_t dcc_occ_history_size(const dcc_ctx* ctx);
/* Drop every history entry with tn <= tn_floor.  The reference never frees
 * history (occ.cpp:277-286 only pushes); an entry is visible to
 * a window (start_tn, finish_tn] only if tn > start_tn, so a caller that knows
 * no txn will ever validate with start_tn < tn_floor can bound the history. */
int dcc_occ_history_trim(dcc_ctx* ctx, uint64_t tn_floor);
/* Copy the history's (key, tn) pairs to host arrays of cap entries (any
 * order); *out_n = the history size.  DCC_ERANGE when cap is too small. */
int dcc_occ_history_export(dcc_ctx* ctx, uint64_t* keys, uint64_t* tn, uint64_t cap,
                           uint64_t* out_n);
/* The commit counter `tnc` (occ.h:67). */
int dcc_occ_set_tnc(dcc_ctx* ctx, uint64_t tnc);
uint64_t dcc_occ_get_tnc(const dcc_ctx* ctx);

/* Captured-snapshot validation.  A live, genuinely
 * concurrent run records, for every validating txn, what its critical section
 * saw (occ.cpp:137-158): the history head and the active list.  Every txn is
 * then validated independently and in parallel against exactly that snapshot,
 * reproducing central_validate's decision (occ.cpp:116-239) bit for bit.
 *   hist_top[i]   tn of the history head at i's critical section: entries with
 *                 tn > hist_top[i] were pushed later and are invisible to i.
 *                 NULL = the whole context history is visible.
 *   active_off    [n_txn+1] CSR; active_idx[active_off[i] .. active_off[i+1])
 *                 are the batch indices of the txns whose write sets were on the
 *                 active list (finish_active, occ.cpp:146-150) when i entered.
 * The history itself is the context's (dcc_occ_history_append).  start_tn /
 * finish_tn of the batch open the window exactly as in central_validate
 * (checked against the read set only, occ.cpp:167-180); the active check is
 * against the read set, then the write set (occ.cpp:185-199).  Pointers are
 * device memory when batch->flags has DCC_DEVICE_PTRS (then out_rc too).
 * Nothing is committed: central_finish of a live run is the caller's.
 * Stats: n_commit, n_abort, n_readonly, nnz_w, device_ms, total_ms, alg_bytes. */
typedef struct dcc_occ_snapshot {
  const uint64_t* hist_top;   /* [n_txn] or NULL */
  const uint32_t* active_off; /* [n_txn+1] */
  const uint32_t* active_idx; /* [active_off[n_txn]] indices < n_txn */
} dcc_occ_snapshot;
int dcc_occ_validate_snapshot(dcc_ctx* ctx, const dcc_batch* batch, const dcc_occ_snapshot* snap,
                              uint8_t* out_rc, dcc_stats* out_stats);

/* ----------------------------------------------------------------- MaaT */
/* MaaT epoch validation.  Epoch model: every txn of
 * the batch is initialised in the time table ([0, UINT64_MAX], RUNNING;
 * worker_thread.cpp:503-508) and performs its Row_maat accesses in index
 * order (RD -> read, WR -> prewrite, XP/SCAN -> none; with
 * DCC_MAAT_READ_AND_PREWRITE every access does read_and_prewrite,
 * row_maat.cpp:38-164); then, in index order, each txn runs Maat::validate
 * and find_bound (maat.cpp:29-191; the node is the home node) and commits
 * (Row_maat::commit with the forward validation of the later txns still on
 * its rows, row_maat.cpp:189-314) or aborts (row_maat.cpp:167-187).
 *   out_rc[i]        = DCC_RC_RCOK or DCC_RC_ABORT
 *   out_commit_ts[i] = commit_timestamp (the lower bound find_bound picks) or 0
 * Row timestamps (timestamp_last_read / _write, row_maat.h:38-39) persist in
 * the context across epochs; rows never seen start at 0.
 * Stats: n_commit, n_abort, nnz_w, rounds (of the GPU fixed point),
 * device_ms, total_ms, alg_bytes (dcc_maat_alg_bytes). */
int dcc_maat_validate_epoch(dcc_ctx* ctx, const dcc_batch* batch, uint8_t* out_rc,
                            uint64_t* out_commit_ts, dcc_stats* out_stats);
/* Row timestamps: seed (overwrite) / read (0 for unknown rows) / forget.
 * Host arrays of n entries. */
int dcc_maat_rows_set(dcc_ctx* ctx, const uint64_t* keys, const uint64_t* last_read,
                      const uint64_t* last_write, uint64_t n);
int dcc_maat_rows_get(dcc_ctx* ctx, const uint64_t* keys, uint64_t* last_read,
                      uint64_t* last_write, uint64_t n);
int dcc_maat_rows_clear(dcc_ctx* ctx);
uint64_t dcc_maat_rows_size(const dcc_ctx* ctx);
/* Algorithmic bytes of one MaaT epoch: 4(N+1) offsets + 9 nnz (key, type)
 * + 24 nnz (row slot: key, last read, last write) + 8 nnz (timestamp update)
 * + N (RC) + 8 N (commit timestamp). */
uint64_t dcc_maat_alg_bytes(uint64_t n_txn, uint64_t nnz);

/* --------------------------------------------------------------- Calvin */
/* Epoch lock ordering: the result equals the epoch's txns calling
 * acquire_locks (ycsb_txn.cpp:49-88) in sequence order against an empty
 * Row_lock table in CALVIN mode (row_lock.cpp:52-216), with per-txn row
 * de-duplication (txn.cpp:778-782) and RD/SCAN->SH, else EX (row.cpp:191).
 *   out_group[a] = grant group of request a on its row: 0 = granted at
 *                  acquire, g = granted when group g-1 has fully released
 *                  (lock_release promotion, row_lock.cpp:317-357);
 *                  DCC_GROUP_NONE for a de-duplicated request.  May be NULL.
 *   out_rc[i]    = DCC_RC_RCOK if every request is in group 0, else DCC_RC_WAIT
 *                  (acquire_locks' return).
 *   out_wave[i]  = wave in which txn i runs when every txn releases all its
 *                  locks one wave after it became ready (may be NULL).
 * batch->order (may be NULL = index order) is the sequencer's order key
 * (origin << 32 | seq); ties keep index order.
 * n_txn < 2^25.  Stats: n_commit = txns ready at acquire (RCOK), n_abort =
 * txns that WAIT, nnz_w = EX requests, rounds = number of waves (0 when
 * out_wave is NULL). */
int dcc_calvin_order_epoch(dcc_ctx* ctx, const dcc_batch* batch, uint32_t* out_group,
                           uint8_t* out_rc, uint32_t* out_wave, dcc_stats* out_stats);

/* Rows still locked when the epoch starts.  Releases are asynchronous
 * (Row_lock::lock_release, row_lock.cpp:219-372), so the lock thread may
 * acquire an epoch while rows are still owned, or queued for, by txns of an
 * earlier epoch.  The held prefix lists those requests per row in FIFO order:
 * the current owners first, then the waiters (any interleaving of rows; the
 * order among one row's requests is the queue order).  They enter the same
 * per-row order ahead of the epoch's requests, so:
 *   out_group[a] counts group boundaries from the row's owners (group 0 = the
 *                current owners; an epoch request in group 0 joins them),
 *   out_rc[i]    = RCOK iff every request of txn i joins its row's owners.
 * Equal to replaying the prefix requests, then the epoch, through Row_lock in
 * CALVIN mode.  Host arrays, or device arrays when batch->flags has
 * DCC_DEVICE_PTRS.  Wave levels need an empty table: out_wave must be NULL
 * (DCC_ENOTSUP otherwise).  Key-sharded: each rank passes its own rows. */
typedef struct dcc_calvin_held {
  uint64_t n;              /* held requests                                 */
  const uint64_t* keys;    /* [n] rows                                      */
  const uint8_t* acctype;  /* [n] access_t (RD/SCAN -> SH, else EX)         */
} dcc_calvin_held;
int dcc_calvin_order_epoch_held(dcc_ctx* ctx, const dcc_batch* batch, const dcc_calvin_held* held,
                                uint32_t* out_group, uint8_t* out_rc, uint32_t* out_wave,
                                dcc_stats* out_stats);

/* ------------------------------------------------------- NO_WAIT (2PL) */
/* Epoch lock acquisition under CC_ALG NO_WAIT: the result equals the txns of
 * the batch calling get_row for their accesses, txn by txn in index order and
 * access by access in list order, against a Row_lock table in NO_WAIT mode
 * (storage/row.cpp:226-238, concurrency_control/row_lock.cpp:52-216):
 * RD/SCAN request LOCK_SH, everything else LOCK_EX (row.cpp:228); a request
 * conflicts iff the row's lock_type is not LOCK_NONE and either side is EX
 * (conflict_lock, row_lock.cpp:374-381); the first conflicting request aborts
 * the txn (row_lock.cpp:86-90), which releases what it took (cleanup ->
 * lock_release, system/txn.cpp:747-761, row_lock.cpp:240-256) and requests
 * nothing more; a txn that gets every lock holds them all to the end of the
 * epoch (strict 2PL).  NO_WAIT keeps no owner list (row_lock.cpp:176-182), so
 * a txn naming a row twice with EX on either side aborts on its own second
 * request; two SH requests on one row are fine.
 *   held            rows still locked by txns of earlier epochs, (key, access
 *                   type) pairs: EX-held if any entry of the row is EX, else
 *                   SH-held; they enter the table before txn 0 and are never
 *                   released.  May be NULL.
 *   out_rc[i]       = DCC_RC_RCOK (holds every lock) or DCC_RC_ABORT
 *   out_conflict[i] = for an aborted txn the ordinal within the txn (0-based
 *                     from offsets[i]) of the first access whose lock_get
 *                     returned Abort (the request txn.cpp:803-816 aborts at);
 *                     DCC_ACCESS_NONE for a committed txn.  May be NULL.
 * start_tn / finish_tn / order of the batch are ignored.  With DCC_DEVICE_PTRS
 * the batch, the held arrays and the outputs are device memory.  The lock
 * table lives for the call only: the caller carries held rows from one epoch
 * to the next.  Without DCC_SHARD_SELF in batch->flags the epoch is one GPU's:
 * a dcc_init_multi context runs it on rank 0, a communicator of more than one
 * rank is DCC_ENOTSUP.
 * With DCC_SHARD_SELF the epoch is key-sharded over the ranks of the context's
 * communicator (dcc_comm_init, dcc_comm_init_host, the one-rank RCCL clique of
 * DCC_OPT_COMM_SOLO) or the sub-contexts of a dcc_init_multi context.  Every
 * rank passes the same whole batch and the same whole held list, with the same
 * out_conflict choice; rank r keeps the rows with dcc_key_shard(key, R) == r,
 * held rows included, in a lock table sized from its own requests and held
 * rows.  Every rank returns the whole out_rc / out_conflict, identical on all
 * ranks and equal to the one-GPU epoch's.  The call is a collective: one
 * byte-MAX all-reduce of n_txn bytes per round enqueued and one more for
 * out_conflict; every rank checks the whole batch and the whole held list
 * before its first, so a malformed epoch is DCC_EINVAL on every rank alike.
 * A dcc_init_multi context runs one host thread per rank, returns rank 0's
 * outputs (host outputs: after comparing every rank's; a difference is
 * DCC_EIO) and, when a rank fails, ends the others' exchanges instead of
 * leaving them waiting.  Stats are the whole batch's on every rank, n_shards
 * the ranks that took part, device_ms of a dcc_init_multi context the maximum
 * over its ranks.  On a context without a communicator (or with one rank and
 * no DCC_OPT_COMM_SOLO) the flag is ignored.  Out of scope: the lock-table
 * handle (dcc_locktab_lock_epoch behaves as described there whatever the
 * flag says), exchanging in list order instead of n_txn bytes per round, and
 * pipelining sharded epochs; TIMESTAMP, MVCC, WAIT_DIE and MaaT are not
 * key-sharded.
 * Isolation (DCC_ISO_* in batch->flags): the same replay with the reference's
 * early releases, the YCSB behaviour for every batch (TPC-C in the reference
 * never calls release_last_row_lock; that leak is not modelled).
 *   READ_COMMITTED    a granted RD/SCAN is released at once, so a read never
 *                     blocks a later writer; an abort releases the txn's EX
 *                     rows, a committed txn holds its EX rows.  Within a txn
 *                     RD then WR of one row is fine, WR then RD and WR then WR
 *                     abort at the second.
 *   READ_UNCOMMITTED  every granted lock is released at once: a txn aborts
 *                     only on the held prefix (a row EX-held, or held and the
 *                     access EX); without `held` every txn commits.  rounds 0.
 * `held` stays a literal statement of the table before txn 0 at every level
 * (an SH entry is an SH lock): a READ_COMMITTED caller passes what its earlier
 * txns still hold, their EX rows.  An isolation bit on an epoch that would run
 * key-sharded (DCC_SHARD_SELF on a communicator of more than one rank, on
 * DCC_OPT_COMM_SOLO, or on a dcc_init_multi context of more than one rank) is
 * DCC_ENOTSUP on every rank, before any collective.
 * Stats: n_commit, n_abort, nnz_w (EX requests), n_readonly (txns with no EX
 * request), rounds, device_ms, total_ms, alg_bytes (dcc_nowait_iso_alg_bytes);
 * with profiling phase_ms: 0 = table build, 1 = round 1, 2 = rounds >= 2,
 * 3 = RC / conflict pass. */
#define DCC_ACCESS_NONE 0xFFFFFFFFu
int dcc_nowait_lock_epoch(dcc_ctx* ctx, const dcc_batch* batch, const dcc_calvin_held* held,
                          uint8_t* out_rc, uint32_t* out_conflict, dcc_stats* out_stats);
/* Algorithmic bytes of one NO_WAIT epoch: 4(N+1) offsets + 9 nnz (key, type)
 * + 16 nnz (one lock-table slot per request) + N (RC) [+ 4N conflict]. */
uint64_t dcc_nowait_alg_bytes(uint64_t n_txn, uint64_t nnz, int with_conflict);
/* The same at the level in `flags` (DCC_ISO_*): SERIALIZABLE and
 * READ_COMMITTED equal dcc_nowait_alg_bytes (a read still probes one slot);
 * READ_UNCOMMITTED drops the 16 nnz when held_n == 0 (no table is built). */
uint64_t dcc_nowait_iso_alg_bytes(uint64_t n_txn, uint64_t nnz, uint64_t held_n, int with_conflict,
                                  uint32_t flags);

/* ------------------------------------------------ TIMESTAMP (basic T/O) */
/* Epoch under CC_ALG TIMESTAMP with one txn in flight at a time: the result
 * equals the txns of the batch running in index order, each calling get_row
 * for its accesses in list order and then committing or aborting before the
 * next txn starts, against Row_ts (concurrency_control/row_ts.cpp:167-266,
 * storage/row.cpp:239-282, 371-390, system/txn.cpp:700-761).  ts[i] is the
 * txn's timestamp (txn->get_timestamp()): any u64, in any order, ties allowed;
 * every comparison is the reference's unsigned `<`.  Per row, wts and rts
 * (row_ts.cpp:27-28) persist in the context across epochs; rows never seen
 * are (0, 0).  Per access (row.cpp:252-258):
 *   RD / SCAN  R_REQ: abort if ts < wts (row_ts.cpp:176), else
 *              rts = max(rts, ts) (:188-189);
 *   WR         P_REQ then R_REQ: abort if ts < rts or ts < wts (:193, :200;
 *              TS_TWR is false, config.h:123), else rts = max(rts, ts);
 *   XP         no request.
 * The first aborting access ends the txn; its cleanup sends XP_REQ for the WR
 * accesses made (txn.cpp:700-704, row.cpp:380-384), which only drops the
 * prewrite: the rts bumps of an aborted txn stay, wts is untouched.  A txn
 * that passes every access commits, and each of its WR accesses sends W_REQ:
 * wts = max(wts, ts) (row_ts.cpp:237-239).  In this model no request is ever
 * buffered or returns WAIT; Row_ts's buffered requests
 * (concurrent txns) are dcc_tso_access_epoch / dcc_tso_finish below; TS_TWR
 * is out of scope.
 *   ts              [n_txn] timestamps; NULL is DCC_EINVAL
 *   out_rc[i]       = DCC_RC_RCOK or DCC_RC_ABORT
 *   out_conflict[i] = for an aborted txn the ordinal within the txn (0-based
 *                     from offsets[i]) of the access that aborted it;
 *                     DCC_ACCESS_NONE for a committed txn.  May be NULL.
 * start_tn / finish_tn / order of the batch are ignored.  With DCC_DEVICE_PTRS
 * the batch, ts and the outputs are device memory.  A rejected batch
 * (malformed offsets, a txn longer than MAX_ROW_PER_TXN, the reserved key:
 * DCC_EINVAL) leaves the row table unchanged.  One GPU: a dcc_init_multi
 * context runs the epoch on rank 0; a communicator of more than one rank is
 * DCC_ENOTSUP.
 * Stats: n_commit, n_abort, nnz_w (WR accesses), n_readonly (txns with no WR
 * access), rounds, device_ms, total_ms, alg_bytes (dcc_tso_alg_bytes); with
 * profiling phase_ms: 0 = sort / build, 1 = round 1, 2 = rounds >= 2,
 * 3 = final pass + table update. */
int dcc_tso_validate_epoch(dcc_ctx* ctx, const dcc_batch* batch, const uint64_t* ts, uint8_t* out_rc,
                           uint32_t* out_conflict, dcc_stats* out_stats);
/* Row timestamps: seed (overwrite) / read (0 for unknown rows) / forget.
 * Host arrays of n entries.  The table holds every row that was seeded or
 * named by an accepted batch, reached by an executed access or not (such a row
 * is (0, 0), which reads the same as an unknown one): dcc_tso_rows_size. */
int dcc_tso_rows_set(dcc_ctx* ctx, const uint64_t* keys, const uint64_t* wts, const uint64_t* rts,
                     uint64_t n);
int dcc_tso_rows_get(dcc_ctx* ctx, const uint64_t* keys, uint64_t* wts, uint64_t* rts, uint64_t n);
int dcc_tso_rows_clear(dcc_ctx* ctx);
uint64_t dcc_tso_rows_size(const dcc_ctx* ctx);
/* Algorithmic bytes of one TIMESTAMP epoch: 4(N+1) offsets + 8N timestamps
 * + 9 nnz (key, type) + 24 nnz (one row: key, wts, rts, per access) + N (RC)
 * [+ 4N conflict]. */
uint64_t dcc_tso_alg_bytes(uint64_t n_txn, uint64_t nnz, int with_conflict);

/* -------------------------------------------- TIMESTAMP with txns in flight */
/* Row_ts with its buffers (readreq, prereq, writereq and the cached min_rts /
 * min_pts / min_wts; row_ts.cpp:64-165, :167-323) as two calls, the split of
 * the in-flight MVCC calls below: an epoch that only sends requests -- it
 * decides pass, wait or abort for every access and nothing finishes inside it
 * -- and a finish the caller makes between epochs for the txns that are done,
 * which raises wts, drops prewrites and promotes buffered reads as
 * Row_ts::update_buffer does.  When other txns finish is thereby an input.
 * DESIGN.md §8t has the arguments.
 *
 * State.  The WAIT_DIE / in-flight MVCC calls' (see there): caller-owned
 * rc[n_txn] (u8, the same five bytes), pos[n_txn] (u32) and ts[n_txn] over a
 * batch the caller keeps, so that dcc_waitdie_carry and dcc_batch_select move
 * a TIMESTAMP population unchanged.  ts[i] is any u64, in any order, ties
 * allowed, as for dcc_tso_validate_epoch; every comparison is the reference's
 * unsigned `<` / `>`.  No value is reserved: a prewrite at UINT64_MAX behaves
 * exactly as no prewrite, because min_pts is UINT64_MAX either way
 * (row_ts.cpp:31, :157).  With len the txn's access count:
 *   a txn that is not GONE holds one pending prewrite (ts[i]) on the row of
 *   each of its WR accesses in [0, pos);
 *   a WAIT txn (pos < len) has a buffered read on the row of access pos, and if
 *   that access is a WR also that access's prewrite (P_REQ precedes R_REQ,
 *   row.cpp:252-258);
 *   a new txn is (RUN, 0); RCOK has pos == len.
 * wts and rts of each row are the context's TIMESTAMP row table above, shared
 * with dcc_tso_rows_set / get / clear / size and dcc_tso_validate_epoch.
 * dcc_tso_validate_epoch ignores pending prewrites: calling it on a context
 * while a population holds any is the caller's error.
 *
 * dcc_tso_access_epoch.  The RUN txns run in index order, each from pos[i], in
 * list order (row_ts.cpp:167-208), against the state of all other txns, the
 * prefixes the RUN txns hold and what the RUN txns before them did:
 *   RD/SCAN   R_REQ: abort iff ts < wts (:176); else wait iff ts > the least
 *             pending prewrite ts of the row (:178); else rts = max(rts, ts)
 *             (:188-189);
 *   WR        P_REQ: abort iff ts < rts or ts < wts (:193, :200; TS_TWR is
 *             false); otherwise the prewrite becomes pending (:204) and R_REQ
 *             follows.  The wait test is strict, so a txn's own prewrite and
 *             ties never block it;
 *   XP        sends nothing.
 * First abort: (ABORT, ordinal); first wait: (WAIT, ordinal), out_conflict[i]
 * the ordinal in both; past the last access (RCOK, len), DCC_ACCESS_NONE.  Txns
 * that are not RUN are unchanged, their out_conflict is DCC_ACCESS_NONE.
 * Cleanup is deferred: an aborted txn keeps the prewrites it made, old and new,
 * until a finish releases it, and its rts bumps stay.  wts does not change
 * inside an epoch.
 *
 * dcc_tso_finish.  leave[i] != 0 marks the txns that go.  An RCOK leaver
 * commits: W_REQ per WR access, wts = max(wts, ts) (:236-244), and the prewrite
 * goes.  An ABORT or RUN leaver aborts: XP_REQ per WR access in [0, pos)
 * (:249-253).  A WAIT leaver is DCC_EINVAL (waits run from larger to smaller
 * ts, so none lasts for ever); a GONE one is ignored.  The leavers become GONE.
 * Then update_buffer (:268-323) per row: every buffered read with ts <= the
 * least remaining pending prewrite ts executes: rts = max(rts, ts), and (WAIT,
 * p) becomes (RUN, p + 1); there is no abort check at promotion, as in the
 * reference.  A leaver's W_REQ is never buffered (writereq stays empty, so
 * update_buffer's write branch, :300-320, is never reached),
 * and applying all wts maxima and then promoting equals releasing the leavers
 * one at a time, in any order.  *out_left (host, may be NULL) = the leavers
 * that were not GONE, *out_promoted (host, may be NULL) = the promoted txns.
 *
 * Arrays (host or DCC_DEVICE_PTRS), compact batch forms, rejections (DCC_EINVAL
 * with nothing written and the rows unchanged: malformed offsets, the reserved
 * key, a txn longer than MAX_ROW_PER_TXN, NULL ts / rc / pos (leave for a
 * finish), an rc byte outside the five states, pos > len, RCOK with pos != len,
 * WAIT with pos >= len, a WAIT leaver), DCC_ENOTSUP for an epoch whose keys
 * vary in all 64 bits, for a communicator of more than one rank and for
 * DCC_ISO_* bits, rank 0 of a dcc_init_multi context and pipelined OCC epochs
 * completing first are all exactly as the in-flight MVCC pair's.
 * Stats of the epoch: n_commit / n_abort / n_survivors = the txns that became
 * RCOK / ABORT / WAIT; nnz_w = WR requests (the WR accesses at or past pos of
 * the RUN txns), n_readonly = RUN txns with none; rounds, device_ms, total_ms,
 * alg_bytes; phase_ms as dcc_waitdie_lock_epoch.  Stats of the finish:
 * n_commit = leavers, n_survivors = promoted, device_ms, total_ms. */
int dcc_tso_access_epoch(dcc_ctx* ctx, const dcc_batch* batch, const uint64_t* ts, uint8_t* rc, uint32_t* pos,
                         uint32_t* out_conflict /* may be NULL */, dcc_stats* out_stats);
int dcc_tso_finish(dcc_ctx* ctx, const dcc_batch* batch, const uint64_t* ts, uint8_t* rc, uint32_t* pos,
                   const uint8_t* leave, uint64_t* out_left, uint64_t* out_promoted /* host, may be NULL */,
                   dcc_stats* out_stats);
/* Algorithmic bytes of one access epoch: dcc_waitdie_alg_bytes (the 24-B row
 * aggregate being rts, least pending prewrite, wts). */
uint64_t dcc_tso_access_alg_bytes(uint64_t n_txn, uint64_t nnz, int with_conflict);

/* ------------------------------------------------------------------ MVCC */
/* Epoch under CC_ALG MVCC with one txn in flight at a time, the model of the
 * TIMESTAMP epoch above: the txns of the batch run in index order, each
 * calling get_row for its accesses in list order (WR: P_REQ then R_REQ; RD /
 * SCAN: R_REQ; XP: nothing) and then committing or aborting before the next
 * txn starts, against Row_mvcc (concurrency_control/row_mvcc.cpp:198-334,
 * storage/row.cpp:239-282, 371-390, system/txn.cpp:700-761).  ts[i] is any u64
 * in [1, 2^64-2], in any order, ties allowed; 0 (Row_mvcc::conflict's "none",
 * row_mvcc.cpp:208-229, and the base row below) and UINT64_MAX (DCC_VTS_NONE)
 * are DCC_EINVAL.  In this model (DESIGN.md §8l has the argument):
 *   R_REQ   never waits and never aborts; it returns the newest-inserted
 *           version with wts <= ts, else the base row (:266-270), and enters
 *           ts into the row's read history;
 *   P_REQ   aborts iff ts < rts, the largest read timestamp of the row
 *           (:218-239; every write timestamp is also a read timestamp, so no
 *           write lies between ts and the next read above it);
 *   W_REQ   (per WR access of a committed txn) installs the version ts;
 *   XP_REQ  (per WR access of an aborted txn) drops the prewrite: the rts
 *           bumps of an aborted txn stay, it installs no version.
 * A txn's own writes are installed at its commit: its later reads of the row
 * do not see them.  A row's versions are non-decreasing in ts in commit order.
 * Per row the latest version and rts, and every version (its timestamp; row
 * data and the writer's identity are not tracked), persist in the context
 * across epochs.  There is no seeding call: state is reached by running
 * epochs, which keeps rts >= latest version.
 *   ts              [n_txn] timestamps; NULL is DCC_EINVAL
 *   out_rc[i]       = DCC_RC_RCOK or DCC_RC_ABORT
 *   out_conflict[i] = for an aborted txn the ordinal of the WR access that
 *                     aborted it; DCC_ACCESS_NONE for a committed txn.  May be
 *                     NULL.
 *   out_vts[a]      = [nnz], batch order: the timestamp of the version access
 *                     a's R_REQ returned (a WR that passes reports the version
 *                     it copied); DCC_VTS_BASE for the base row; DCC_VTS_NONE
 *                     for an XP access and for an access that was not executed
 *                     (at or after its txn's abort ordinal).  May be NULL (no
 *                     version is resolved then).
 * Batch forms, DCC_DEVICE_PTRS, multi-GPU contexts (rank 0), communicators of
 * more than one rank (DCC_ENOTSUP) and pipelined OCC epochs in flight are
 * handled as by dcc_tso_validate_epoch.  A rejected batch (malformed offsets,
 * a txn longer than MAX_ROW_PER_TXN, the reserved key, a ts of 0 or
 * UINT64_MAX: DCC_EINVAL) leaves rows and versions unchanged.  An epoch that
 * fails behind its decisions (DCC_EIO) leaves the rows' values and the
 * versions as they were; rows the batch named may have entered the table as
 * (0, 0), which reads as unknown.
 * Stats: as dcc_tso_validate_epoch, except n_survivors = the accesses whose
 * version was resolved by search (0 without out_vts) and phase_ms[3] = final
 * pass, lookups and store merge; alg_bytes is dcc_mvcc_alg_bytes. */
#define DCC_VTS_BASE 0ull
#define DCC_VTS_NONE 0xFFFFFFFFFFFFFFFFull
int dcc_mvcc_validate_epoch(dcc_ctx* ctx, const dcc_batch* batch, const uint64_t* ts, uint8_t* out_rc,
                            uint32_t* out_conflict, uint64_t* out_vts, dcc_stats* out_stats);
/* (latest version, rts) of n rows into host arrays; a row with no version has
 * wts 0, an unknown row is (0, 0).  dcc_mvcc_rows_size: the rows accepted
 * batches named. */
int dcc_mvcc_rows_get(dcc_ctx* ctx, const uint64_t* keys, uint64_t* wts, uint64_t* rts, uint64_t n);
uint64_t dcc_mvcc_rows_size(const dcc_ctx* ctx);
/* The versions in the store, and all of them as (key, ts) pairs sorted by
 * (key, ts) into host arrays of cap entries (either may be NULL); *n_out
 * (may be NULL) = their number; cap smaller than that is DCC_ERANGE with
 * nothing written. */
uint64_t dcc_mvcc_versions_size(const dcc_ctx* ctx);
int dcc_mvcc_versions_export(dcc_ctx* ctx, uint64_t* keys, uint64_t* ts, uint64_t cap, uint64_t* n_out);
/* clear_history(W_REQ, ts_floor) (row_mvcc.cpp:42-73) of every row: a version
 * is dropped iff the next newer version of its row also has ts < ts_floor, so
 * the newest version below the floor stays (:308-320).  The caller guarantees
 * that no later txn has ts < ts_floor; a read below the floor gets whatever
 * the kept versions give.  rts is a maximum and needs no trim.  The
 * reference's automatic trigger (whis_len > HIS_RECYCLE_LEN) is not modelled:
 * trimming is this call.  *n_dropped may be NULL. */
int dcc_mvcc_trim(dcc_ctx* ctx, uint64_t ts_floor, uint64_t* n_dropped);
/* Forget rows and versions together. */
int dcc_mvcc_clear(dcc_ctx* ctx);
/* Algorithmic bytes of one MVCC epoch: dcc_tso_alg_bytes (the 24-B row being
 * key, latest version, rts) [+ 8 nnz versions out].  The store's traffic
 * (lookups, the merge of store + new versions) depends on its size and is not
 * counted. */
uint64_t dcc_mvcc_alg_bytes(uint64_t n_txn, uint64_t nnz, int with_conflict, int with_vts);

/* ------------------------------------------------ MVCC with txns in flight */
/* Row_mvcc with its buffers (readreq_mvcc, prereq_mvcc; row_mvcc.cpp:95-171,
 * :242-364) as two calls, the split of the WAIT_DIE calls below: an epoch that
 * only sends requests -- it decides pass, wait or abort for every access and
 * nothing finishes inside it -- and a finish the caller makes between epochs
 * for the txns that are done, which installs versions, drops prewrites and
 * promotes buffered reads as Row_mvcc::update_buffer does.  When other txns
 * finish is thereby an input.  DESIGN.md §8r has the arguments.
 *
 * State.  The WAIT_DIE calls' (see there): caller-owned rc[n_txn] (u8),
 * pos[n_txn] (u32) and ts[n_txn] over a batch the caller keeps, with the same
 * five bytes DCC_WD_RUN, DCC_RC_RCOK, DCC_RC_WAIT, DCC_RC_ABORT, DCC_WD_GONE, so
 * that dcc_waitdie_carry and dcc_batch_select move an MVCC population
 * unchanged.  ts[i] of a txn that is not GONE is any u64 in [1, 2^64-2], in any
 * order, ties allowed.  With len the txn's access count:
 *   a txn that is not GONE holds one pending prewrite (ts[i]) on the row of
 *   each of its WR accesses in [0, pos);
 *   a WAIT txn (pos < len) has a buffered read on the row of access pos, and if
 *   that access is a WR also that access's prewrite (P_REQ precedes R_REQ,
 *   row.cpp:252-258);
 *   a new txn is (RUN, 0); RCOK has pos == len.
 * rts, the latest version and every version of each row are the context's MVCC
 * rows and store above, shared with dcc_mvcc_validate_epoch, dcc_mvcc_rows_get,
 * dcc_mvcc_versions_*, dcc_mvcc_trim and dcc_mvcc_clear.
 * dcc_mvcc_validate_epoch ignores pending prewrites: calling it on a context
 * while a population holds any is the caller's error.
 * vts (may be NULL) is a caller-kept [nnz] array in batch order: each call
 * writes the entries of the accesses whose R_REQ it executes (the version's
 * timestamp, DCC_VTS_BASE for the base row) and leaves the others alone.
 *
 * dcc_mvcc_access_epoch.  The RUN txns run in index order, each from pos[i], in
 * list order, against the state of all other txns, the prefixes the RUN txns
 * hold and what the RUN txns before them did:
 *   WR        P_REQ aborts iff ts < rts of the row; otherwise the prewrite
 *             becomes pending and R_REQ follows;
 *   RD/SCAN   R_REQ only; XP sends nothing;
 *   R_REQ     waits iff some pending prewrite of the row is below ts (the txn's
 *             own prewrites and ties never block); otherwise it returns the
 *             largest version <= ts, or the base row, and rts = max(rts, ts).
 * First abort: (ABORT, ordinal); first wait: (WAIT, ordinal), out_conflict[i]
 * the ordinal in both; past the last access (RCOK, len), DCC_ACCESS_NONE.  Txns
 * that are not RUN are unchanged, their out_conflict is DCC_ACCESS_NONE.
 * Cleanup is deferred: an aborted txn keeps the prewrites it made, old and new,
 * until a finish releases it, and its rts bumps stay, as in the reference,
 * whose cleanup is not atomic with the abort decision.  The reference's caps
 * g_max_read_req / g_max_pre_req (the txns in flight) are not modelled.
 *
 * dcc_mvcc_finish.  leave[i] != 0 marks the txns that go.  An RCOK leaver
 * commits: W_REQ per WR access installs version ts.  An ABORT or RUN leaver
 * aborts: XP_REQ per WR access in [0, pos).  A WAIT leaver is DCC_EINVAL
 * (wait-for edges run from larger to smaller ts, so no txn waits for ever); a
 * GONE one is ignored.  The leavers become GONE.  Then per row a buffered read
 * with ts <= the least remaining pending prewrite ts is promoted
 * (debuffer_req(R_REQ), :143-167): it reads the largest version <= ts of the
 * store after the installs, raises rts, and (WAIT, p) becomes (RUN, p + 1); a
 * RUN txn at pos == len turns RCOK in the next epoch.  This equals releasing
 * the leavers one at a time in index order, newest access first.  *out_left
 * (host, may be NULL) = the leavers that were not GONE, *out_promoted (host, may
 * be NULL) = the promoted txns.
 *
 * rc / pos / vts are updated in place.  With DCC_DEVICE_PTRS every array is
 * device memory, otherwise a host array.  Compact batch forms are accepted;
 * start_tn / finish_tn / order are ignored.  DCC_EINVAL, with nothing written:
 * malformed offsets, the reserved key, a txn longer than MAX_ROW_PER_TXN, NULL
 * ts / rc / pos (leave for a finish), an rc byte outside the five states, pos >
 * len, RCOK with pos != len, WAIT with pos >= len, a ts of 0 or UINT64_MAX of a
 * txn that is not GONE, a WAIT leaver.  An epoch whose keys vary in all 64 bits
 * is DCC_ENOTSUP (its sort needs one bit next to the row; the finish needs
 * none).  One GPU: a dcc_init_multi context runs on rank 0; a communicator of
 * more than one rank is DCC_ENOTSUP; pipelined OCC epochs in flight complete
 * first.  A call that fails behind its decisions (DCC_EIO) leaves the rows'
 * values and the store as they were.
 * Stats of the epoch: n_commit / n_abort / n_survivors = the txns that became
 * RCOK / ABORT / WAIT; nnz_w = WR requests (the WR accesses at or past pos of
 * the RUN txns), n_readonly = RUN txns with none; rounds, device_ms, total_ms,
 * alg_bytes; phase_ms as dcc_waitdie_lock_epoch.  Stats of the finish:
 * n_commit = leavers, n_survivors = promoted, nnz_w = versions installed,
 * device_ms, total_ms. */
int dcc_mvcc_access_epoch(dcc_ctx* ctx, const dcc_batch* batch, const uint64_t* ts, uint8_t* rc, uint32_t* pos,
                          uint64_t* vts /* [nnz], may be NULL */, uint32_t* out_conflict /* may be NULL */,
                          dcc_stats* out_stats);
int dcc_mvcc_finish(dcc_ctx* ctx, const dcc_batch* batch, const uint64_t* ts, uint8_t* rc, uint32_t* pos,
                    const uint8_t* leave, uint64_t* vts /* may be NULL */, uint64_t* out_left,
                    uint64_t* out_promoted /* host, may be NULL */, dcc_stats* out_stats);
/* Algorithmic bytes of one access epoch: dcc_waitdie_alg_bytes (the 24-B row
 * aggregate being rts, least pending prewrite, latest version) [+ 8 nnz
 * versions out].  The store's traffic is not counted. */
uint64_t dcc_mvcc_access_alg_bytes(uint64_t n_txn, uint64_t nnz, int with_conflict, int with_vts);

/* -------------------------------------------------------------- WAIT_DIE */
/* CC_ALG WAIT_DIE (Row_lock, concurrency_control/row_lock.cpp) as two calls:
 * an epoch that only acquires -- it decides grant, wait or die for every
 * request, nothing finishes inside it -- and a release the caller makes
 * between epochs for the txns that have finished, which promotes waiters as
 * Row_lock::lock_release does (:306-357).  When other txns finish is thereby an
 * input, which is what gives WAIT_DIE exact semantics in epochs.
 *
 * State.  There is no table object: the lock state is two caller-owned per-txn
 * arrays rc[n_txn] (u8) and pos[n_txn] (u32) over a batch the caller keeps,
 * next to ts[n_txn], ts[i] being txn->get_timestamp() (given once, at the
 * txn's first start, worker_thread.cpp:478): any u64, in any order, ties
 * allowed.  RD / SCAN request LOCK_SH, every other access type LOCK_EX
 * (row.cpp:228).  With len the txn's access count:
 *   rc[i]         pos[i]    meaning
 *   DCC_WD_RUN    p <= len  owns accesses [0, p); requests from p on in the
 *                           next epoch.  A new txn is (RUN, 0).
 *   DCC_RC_RCOK   len       owns every access
 *   DCC_RC_WAIT   p < len   owns [0, p); queued on the row of access p
 *   DCC_RC_ABORT  p <= len  died; still owns [0, p) until released (below)
 *   DCC_WD_GONE   ignored   no trace
 * "Owns access q" is one owner entry (type of q, ts[i]) on the row of q.  A
 * row's lock_type is EX if an owner entry is EX, SH if it has owner entries
 * and none is EX, else NONE.  Its waiter queue holds its waiter entries in
 * descending ts, the head being the largest (:133-141); among equal ts the
 * lower txn index is nearer the head (the reference's order there depends on
 * arrival, and it asserts distinct owner timestamps, :107: ties are outside
 * its domain and decided here deterministically).
 *
 * dcc_waitdie_lock_epoch.  The RUN txns run in index order, each calling
 * lock_get for its accesses from pos[i] on, in list order, against the state
 * of all non-RUN txns, the owned prefixes of the RUN txns and what the RUN
 * txns before it left.  A request of txn i, type t, on row K:
 *   conflict (:69-77) iff K has an EX owner entry, or t is EX and K has any
 *   owner entry, or K has a waiter and ts_i < the largest waiter ts;
 *   no conflict: granted, an owner entry is added (:171-196), the txn goes on;
 *   conflict (:91-151): if ts_i > some owner's ts (the least owner ts) the txn
 *   dies: (ABORT, its input pos), out_conflict[i] the access's ordinal; the
 *   owner entries it gained in this epoch are released at once (system/txn.cpp
 *   cleanup -> lock_release) and leave no trace: such a release restores the
 *   row exactly and promotes nothing, because waiters exist only behind a head
 *   that conflicts with lock_type.  Otherwise it waits: (WAIT, ordinal), a
 *   waiter entry is added, out_conflict[i] the ordinal;
 *   past its last access the txn becomes (RCOK, len), out_conflict[i]
 *   DCC_ACCESS_NONE.
 * A txn's own earlier entries on K count as owners like anyone else's (the
 * reference with its asserts compiled out; :106 would trip): RD then WR of one
 * row makes the txn wait on itself when every other owner is younger; two SH
 * requests of one txn on one row give two entries.  Txns that are not RUN are
 * unchanged, their out_conflict is DCC_ACCESS_NONE.
 * Deferred cleanup: a RUN txn that dies with a carried prefix (pos > 0 on
 * input) keeps those owner entries until the caller releases it; releasing
 * them inside the epoch would promote waiters mid-epoch.  This is a legal
 * interleaving of the reference, where the dying worker's cleanup is not atomic
 * with its abort decision and other workers' lock_gets land in between.
 *
 * dcc_waitdie_release.  leave[i] != 0 marks the txns that go; any state may
 * leave (the reference's waiter removal, behind assert(false) at :289-303, is
 * what drops a WAIT txn: a caller needs it for a self-waiter or a timeout).
 * Every entry of every leaver is removed and the leavers become GONE (their pos
 * is left as it was).  Then :317-357 runs on each row with lock_type that of
 * the remaining owner entries: while the queue head does not conflict with
 * lock_type it becomes an owner and lock_type its type -- nothing, the head
 * alone, or a leading run of SH waiters when no EX owner remains.  A promoted
 * (WAIT, p) becomes (RUN, p + 1) (txn_table.restart_txn -> get_row_post_wait,
 * row.cpp:313-321) and resumes in the next epoch; a RUN txn at pos == len turns
 * RCOK there.  Releasing the leavers one at a time with lock_release, in any
 * order, ends in the same state.  *out_left (host, may be NULL) = the leavers
 * that were not GONE, *out_promoted (host, may be NULL) = the promoted txns.
 * States no history reaches (two EX owners, say) are decided by these rules.
 *
 * rc / pos are updated in place.  With DCC_DEVICE_PTRS every array is device
 * memory, otherwise a host array.  Compact batch forms are accepted; start_tn /
 * finish_tn / order are ignored.  DCC_EINVAL, before rc / pos / the outputs
 * are written: malformed offsets, the reserved key, a txn longer than
 * MAX_ROW_PER_TXN, NULL ts / rc / pos (leave for a release), an rc byte outside
 * the five states, pos > len, RCOK with pos != len, WAIT with pos >= len.
 * Keys that vary in all 64 bits are DCC_ENOTSUP (the sort needs one bit next
 * to the row).  One GPU: a dcc_init_multi context runs on rank 0; a
 * communicator of more than one rank is DCC_ENOTSUP; pipelined OCC epochs in
 * flight complete first.
 * Stats of the epoch: n_commit / n_abort / n_survivors = the txns that became
 * RCOK / ABORT / WAIT; nnz_w = EX requests (the EX accesses at or past pos of
 * the RUN txns), n_readonly = RUN txns with none; rounds, device_ms, total_ms,
 * alg_bytes; with profiling phase_ms: 0 = sort / build, 1 = round 1, 2 = rounds
 * >= 2, 3 = final pass.  Stats of the release: n_commit = leavers, n_survivors
 * = promoted, device_ms, total_ms. */
#define DCC_WD_RUN 0x10
#define DCC_WD_GONE 0x11
int dcc_waitdie_lock_epoch(dcc_ctx* ctx, const dcc_batch* batch, const uint64_t* ts, uint8_t* rc, uint32_t* pos,
                           uint32_t* out_conflict /* may be NULL */, dcc_stats* out_stats);
int dcc_waitdie_release(dcc_ctx* ctx, const dcc_batch* batch, const uint64_t* ts, uint8_t* rc, uint32_t* pos,
                        const uint8_t* leave, uint64_t* out_left, uint64_t* out_promoted /* host, may be NULL */,
                        dcc_stats* out_stats);
/* Algorithmic bytes of one WAIT_DIE epoch: 4(N+1) offsets + 13N (ts, rc, pos
 * in) + 9 nnz (key, type) + 24 nnz (one row aggregate per access: owner bits,
 * least owner ts, largest waiter ts) + 5N (rc, pos out) [+ 4N conflict]. */
uint64_t dcc_waitdie_alg_bytes(uint64_t n_txn, uint64_t nnz, int with_conflict);

/* dcc_waitdie_carry.  The population of the next epoch, where the batch lives:
 * the stayers followed by the fresh txns.  A stayer is a txn with rc != GONE,
 * or a GONE txn with revive[i] != 0.  Stayers keep their index order; each is
 * written with its accesses in list order and its ts, rc, pos and src
 * (src_in[i], or i when src_in is NULL, so identities compose over any number
 * of carries); a revived txn is written as (RUN, 0) with the ts it keeps
 * (worker_thread.cpp:478).  The fresh txns keep their order behind the stayers,
 * each as (RUN, 0) with its fresh_ts and src = fresh_src_base + j.  *out_kept
 * (host, may be NULL) = the stayers, *out_n / *out_nnz (host, may be NULL) =
 * the txns / accesses of the output.  Nothing of the input is written; the
 * output arrays must not overlap the inputs.
 *
 * The call changes no decision.  A GONE txn has no trace (above), so dropping
 * it removes nothing an epoch or a release reads; the relative index order of
 * all others is preserved, so the order the RUN txns run in and the waiter
 * queues' ties (lower index nearer the head) do not move: epochs and releases
 * on the carried population decide, txn for txn through src, what they decide
 * on the population that was never compacted.  A revived txn keeps its place
 * among the stayers: the reference restarts an aborted txn at an arbitrary
 * later time (system/abort_queue.cpp), so this is one of its interleavings.
 * A died txn that still owns a prefix is not GONE and is simply kept.
 *
 * Txn length is not limited (the call moves data) and zero-length txns are
 * kept; the epoch rejects what it rejects.  batch and fresh must agree on
 * DCC_DEVICE_PTRS: with it every array of the call is device memory, without
 * it host memory.  Either batch may be in any compact form, independently
 * (DCC_KEYS_U32, DCC_ACCTYPE_2BIT; start_tn / finish_tn / order are ignored);
 * the output is always wide.
 * DCC_EINVAL, nothing written: NULL a, batch, out, ts, rc, pos, out_ts, out_rc
 * or out_pos; fresh without fresh_ts; batch and fresh disagreeing on
 * DCC_DEVICE_PTRS; out->txn_base or out->nnz_base not 0; malformed offsets of
 * either batch (checked on the device before anything indexes with them); an
 * rc byte outside the five states; for a txn that is not GONE pos > len, RCOK
 * with pos != len, WAIT with pos >= len (the rules of the epoch, so an
 * accepted output is a state the epoch accepts) or revive[i] != 0.
 * DCC_ERANGE, nothing written to any output array: stayers + fresh exceed
 * out->cap_txn or out->cap_nnz, or the accesses do not fit a uint32_t; *out_n /
 * *out_nnz / *out_kept then report what was needed.
 * Local: no collective.  A dcc_init_multi context runs it on rank 0's GPU, a
 * context with a communicator as any other; pipelined OCC epochs in flight
 * complete first.  dcc_reserve covers its workspaces: a warmed-up call on a
 * device population allocates nothing.
 * Stats: n_commit = stayers, n_abort = dropped, n_survivors = revived,
 * alg_bytes (dcc_waitdie_carry_alg_bytes), device_ms, total_ms; with profiling
 * phase_ms: 0 = count + state check, 1 = scan, 2 = stayers' scatter, 3 = fresh
 * append. */
struct dcc_select_out; /* the select's output CSR, below */
typedef struct dcc_waitdie_carry_args {
  const dcc_batch* batch;     /* the current population; n_txn may be 0                    */
  const uint64_t* ts;         /* [n_txn]                                                   */
  const uint8_t*  rc;         /* [n_txn] the five WAIT_DIE states                          */
  const uint32_t* pos;        /* [n_txn]                                                   */
  const uint8_t*  revive;     /* [n_txn] or NULL: a GONE txn with revive[i] != 0 re-enters
                                 as (DCC_WD_RUN, 0) with its ts                            */
  const uint32_t* src_in;     /* [n_txn] or NULL (identity): composes like the select's    */
  const dcc_batch* fresh;     /* new arrivals, appended behind the stayers; or NULL        */
  const uint64_t* fresh_ts;   /* [fresh->n_txn]                                            */
  uint32_t fresh_src_base;    /* src of fresh txn j = fresh_src_base + j                   */
  const struct dcc_select_out* out; /* CSR (always wide) + src; txn_base and nnz_base
                                 must be 0; start_tn / finish_tn / order are not written              */
  uint64_t* out_ts; uint8_t* out_rc; uint32_t* out_pos;   /* [out->cap_txn]                */
} dcc_waitdie_carry_args;
int dcc_waitdie_carry(dcc_ctx* ctx, const dcc_waitdie_carry_args* a, uint64_t* out_n,
                      uint64_t* out_nnz, uint64_t* out_kept, dcc_stats* out_stats);
/* Algorithmic bytes of one carry:
 *   offsets, rc and revive of the input, read    4(n_txn+1) + n_txn(1 + with_revive)
 *   per stayer: ts and pos read (12 B), ts, rc,
 *   pos written (13 B)                           25 n_kept
 *   stayers' accesses (key + type, read+written) 18 nnz_kept
 *   fresh offsets and ts read                    4(n_fresh+1) + 8 n_fresh
 *   fresh ts, rc, pos written                    13 n_fresh
 *   fresh accesses                               18 nnz_fresh
 *   output offsets written                       4(n_kept + n_fresh + 1)
 *   src, when with_src                           8 n_kept + 4 n_fresh */
uint64_t dcc_waitdie_carry_alg_bytes(uint64_t n_txn, uint64_t n_kept, uint64_t nnz_kept,
                                     uint64_t n_fresh, uint64_t nnz_fresh, int with_revive, int with_src);

/* ------------------------------ NO_WAIT lock table that lives across epochs */
/* Row_lock's NO_WAIT state where the batches live: a device-resident map
 * row -> (lock_type, owner_cnt) that epochs acquire into and finished txns
 * release from, for the life of the handle.  A row that is absent or has
 * owner_cnt == 0 is LOCK_NONE.
 *
 * dcc_locktab_lock_epoch: the epoch's txns run get_row in index order and list
 * order against the table's current state, exactly as dcc_nowait_lock_epoch
 * defines it (self-conflicts included) with the table's rows as its held
 * prefix: a row with owner_cnt > 0 is held, EX-held iff lock_type == LOCK_EX.
 * out_rc, out_conflict and the stats are those of that call, alg_bytes being
 * dcc_locktab_epoch_alg_bytes.  Aborted txns leave no trace; every request of
 * a committed txn stays in the table: owner_cnt++, lock_type = its type
 * (row_lock.cpp:190-194), so a txn naming a row twice with SH adds 2.  A failed
 * epoch (malformed offsets, reserved key, a txn above MAX_ROW_PER_TXN, no
 * room) leaves the table unchanged.
 *
 * dcc_locktab_release: every access of every txn with rc[i] == want (rc NULL:
 * of every txn) does lock_release (row_lock.cpp:240-256): owner_cnt--, and
 * lock_type = LOCK_NONE at zero.  NO_WAIT keeps no owner list, so the access
 * type plays no part.  The reference's assert(owner_cnt > 0) is an error here:
 * if the releases of ONE CALL together name a row more often than it is held,
 * or name a row the table does not have, the call returns DCC_EINVAL and the
 * table is unchanged (two txns of one call each releasing a row held once
 * fail, although each alone would pass).  Malformed offsets give DCC_EINVAL.
 * Txn length is unbounded.  *out_n / *out_nnz (host memory, may be NULL) are
 * the released txns / accesses.  Stats: n_commit = released txns, n_abort =
 * the others, alg_bytes (dcc_locktab_release_alg_bytes), device_ms, total_ms;
 * with profiling phase_ms: 0 = offsets check, 1 = scratch add, 2 = compare,
 * 3 = apply.
 *
 * Isolation (DCC_ISO_* in batch->flags, per call: one table may see epochs of
 * different levels).  dcc_locktab_lock_epoch decides as dcc_nowait_lock_epoch
 * does at that level; of a committed txn every request stays (SERIALIZABLE),
 * only the EX requests (READ_COMMITTED: the incoming requests of the room rule
 * below are the EX ones), or none (READ_UNCOMMITTED: the table is unchanged).
 * dcc_locktab_release releases every access of a selected txn, only its EX
 * accesses, or none (a valid no-op); *out_nnz counts the accesses released,
 * *out_n the selected txns, and the over-release rule is unchanged.  Both bits
 * together are DCC_EINVAL.  dcc_locktab_acquire_rows, dcc_locktab_release_rows
 * and dcc_locktab_export know no level.
 *
 * dcc_locktab_acquire_rows takes a plain (key, access type) list as the held
 * prefix of dcc_nowait_lock_epoch does: a row is EX if any of its entries is
 * EX, and its count goes up by one per entry.  dcc_locktab_release_rows
 * releases a plain key list under the rule of dcc_locktab_release.
 * dcc_locktab_export writes (key, lock_type, owner_cnt) of the rows with
 * owner_cnt > 0, in any order; lock_type is the reference's lock_t
 * (DCC_LOCK_EX / DCC_LOCK_SH); each output may be NULL; *out_n = the rows
 * held; cap smaller than that is DCC_ERANGE with nothing written.
 * `flags`: DCC_DEVICE_PTRS when the arrays of that call are device memory.
 *
 * Room: the table has 2^k slots, the smallest power of two >= 2 cap_rows, and
 * at most cap_rows of them are ever in use (the load bound: at most half
 * full).  A released row keeps its slot at count 0, so slots fill up with
 * rows that were held once.  Before a lock epoch or an acquire the slots in
 * use plus the incoming requests (an upper bound on the new rows) must fit
 * cap_rows; if they do not, the held rows are first re-inserted into the
 * second table buffer (a rebuild: slots in use = rows held afterwards); if
 * rows held + incoming requests still exceed cap_rows the call returns
 * DCC_ERANGE and the table is logically unchanged.  owner_cnt is a 31-bit count next to the
 * EX bit: the sum of all counts is kept below 2^31 (DCC_ERANGE otherwise).
 *
 * With DCC_DEVICE_PTRS in batch->flags the batch, rc and the outputs are
 * device memory; compact batch forms are accepted.  The table is created with
 * its capacity, lives on the context's GPU (rank 0's of a dcc_init_multi
 * context) and is freed by dcc_destroy if still alive.  A lock epoch under a
 * communicator of more than one rank is DCC_ENOTSUP, with or without
 * DCC_SHARD_SELF: the flag's key-sharded path is dcc_nowait_lock_epoch's
 * alone, and dcc_locktab_lock_epoch ignores it.  No call is a
 * collective.  Pipelined OCC epochs in flight complete first.  Both table
 * buffers, the control words and the staging of host exports are allocated
 * at create, the per-epoch workspaces by dcc_reserve: a warmed-up call on a
 * device batch allocates nothing.  dcc_nowait_lock_epoch and its `held`
 * argument are independent of any table. */
#define DCC_LOCK_EX 0 /* lock_t, system/global.h:289 */
#define DCC_LOCK_SH 1
typedef struct dcc_locktab dcc_locktab;
typedef struct dcc_locktab_params {
  uint64_t cap_rows; /* rows (held or once held) the table has room for; 2^k <= 2^30 slots */
  uint32_t flags;    /* 0 */
  uint32_t reserved;
} dcc_locktab_params;
int dcc_locktab_create(dcc_ctx* ctx, const dcc_locktab_params* params, dcc_locktab** out);
void dcc_locktab_destroy(dcc_locktab* lt);
int dcc_locktab_lock_epoch(dcc_locktab* lt, const dcc_batch* batch, uint8_t* out_rc,
                           uint32_t* out_conflict, dcc_stats* out_stats);
int dcc_locktab_release(dcc_locktab* lt, const dcc_batch* batch, const uint8_t* rc, uint8_t want,
                        uint64_t* out_n, uint64_t* out_nnz, dcc_stats* out_stats);
int dcc_locktab_acquire_rows(dcc_locktab* lt, const dcc_calvin_held* rows, uint32_t flags);
int dcc_locktab_release_rows(dcc_locktab* lt, const uint64_t* keys, uint64_t n, uint32_t flags);
int dcc_locktab_export(dcc_locktab* lt, uint64_t* keys, uint8_t* lock_type, uint32_t* owner_cnt,
                       uint64_t cap, uint32_t flags, uint64_t* out_n);
/* Rows held, slots in use (rows held or once held since the last rebuild or
 * clear), rebuilds over the table's life: host state, no device work.  Each
 * may be NULL. */
int dcc_locktab_size(const dcc_locktab* lt, uint64_t* rows_held, uint64_t* slots_used,
                     uint64_t* rebuilds);
/* Drop every row (the buffers stay). */
int dcc_locktab_clear(dcc_locktab* lt);
/* Device times of the table's own passes in the last lock epoch or acquire
 * run with profiling on: out_ms[0] = seed pass, [1] = grant pass, [2] = the
 * rebuild (0 when there was none). */
int dcc_locktab_pass_ms(const dcc_locktab* lt, double out_ms[3]);
/* Algorithmic bytes of a table epoch: the NO_WAIT epoch's
 * (dcc_nowait_alg_bytes) + 16 nnz (seed: one table slot probed per request)
 * + N (grant: the decision byte) + 25 nnz_granted (grant: key and type read
 * again, one table slot updated). */
uint64_t dcc_locktab_epoch_alg_bytes(uint64_t n_txn, uint64_t nnz, uint64_t nnz_granted,
                                     int with_conflict);
/* Algorithmic bytes of a release of n_sel txns / nnz_sel accesses out of
 * n_txn: 4(N+1) offsets + N (RC) + per released access the key (8), its slot
 * id written and read twice (12) and its table slot touched by each of the
 * three passes (48). */
uint64_t dcc_locktab_release_alg_bytes(uint64_t n_txn, uint64_t n_sel, uint64_t nnz_sel);

/* ------------------------------------------- select by decision (carry) */
/* The next epoch from this one's decisions, where the batch lives: the txns
 * with rc[i] == want (exact equality against any byte value: DCC_RC_ABORT for
 * the retries, DCC_RC_RCOK for the rows still held, DCC_RC_WAIT for Calvin's
 * waiters) are copied into the CSR `out`, in index order, each with its
 * accesses in list order.  The reference hands an aborted txn back to its
 * abort queue (system/abort_queue.cpp) and submits it again; here that is one
 * call between two epochs, with no host copy of a device batch (retried at
 * once; the queue's back-off is dcc_abortq_*, below).
 *   out             where the selection goes (below); its arrays must not
 *                   overlap the batch
 *   rc              [n_txn] decision bytes
 *   src_in          [n_txn] or NULL: out->src gets src_in[i] instead of i, so
 *                   identities compose over any number of retries
 *   *out_n, *out_nnz  selected txns / accesses; always host memory; may be NULL
 * rc, src_in and every array of `out` live where the batch lives: device
 * memory with DCC_DEVICE_PTRS, host memory otherwise.  The batch may be in any
 * compact form (DCC_KEYS_U32, DCC_ACCTYPE_2BIT, DCC_TN_U32); the output is
 * always wide.  Txn length is unbounded (MAX_ROW_PER_TXN does not apply: the
 * call moves data) and zero-length txns are kept.  The offsets are checked on
 * the device before anything indexes with them: malformed ones give DCC_EINVAL.
 * A selection larger than cap_txn / cap_nnz, or one whose nnz_base + accesses
 * does not fit a uint32_t, gives DCC_ERANGE: nothing is written to `out`, and
 * *out_n / *out_nnz report what was needed.  n_txn == 0 gives DCC_OK, zero
 * counts and offsets[txn_base] = nnz_base.
 * Chaining: retries first is select(batch, rc, DCC_RC_ABORT) into the front of
 * the next epoch's arrays, the fresh txns copied in behind out_n / out_nnz;
 * fresh first and retries appended through txn_base / nnz_base needs no host
 * read in between.  select(batch, rc, DCC_RC_RCOK): out->keys / out->acctype
 * with *out_nnz entries are a dcc_calvin_held as they stand.
 * Local: no collective.  A dcc_init_multi context runs it on rank 0's GPU; a
 * context with a communicator attached runs it as any other.  Pipelined OCC
 * epochs in flight complete first.
 * Stats: n_commit = selected txns, n_abort = the rest, alg_bytes
 * (dcc_select_alg_bytes), device_ms, total_ms; with profiling phase_ms:
 * 0 = counting pass, 1 = scan of the tile counts, 2 = scatter. */
typedef struct dcc_select_out {
  uint64_t cap_txn, cap_nnz;   /* room, in txns / accesses, counted from the bases below   */
  uint64_t txn_base, nnz_base; /* selected txn q goes to row txn_base+q, its accesses
                                  start at nnz_base + (accesses of selected txns before it) */
  uint32_t* offsets;           /* [txn_base + cap_txn + 1]; offsets[txn_base] = nnz_base is
                                  written too, so the result chains behind what is there   */
  uint64_t* keys;              /* [nnz_base + cap_nnz]  always the wide form                */
  uint8_t*  acctype;           /* [nnz_base + cap_nnz]  one byte per access                 */
  uint64_t* start_tn, *finish_tn, *order; /* [txn_base + cap_txn] or NULL: gathered when the
                                  batch has the array AND this pointer is set (u64 out)    */
  uint32_t* src;               /* [txn_base + cap_txn] or NULL: source index of each txn   */
} dcc_select_out;
int dcc_batch_select(dcc_ctx* ctx, const dcc_batch* batch, const uint8_t* rc, uint8_t want,
                     const uint32_t* src_in, const dcc_select_out* out,
                     uint64_t* out_n, uint64_t* out_nnz, dcc_stats* out_stats);
/* Algorithmic bytes of one select: 4(N+1) offsets + N (RC) read, 18 per
 * selected access (key + type read and written), 4(n_sel+1) offsets written,
 * 16 n_sel per per-txn array carried (start_tn, finish_tn, order: 8 B read and
 * 8 B written; src is counted the same, a bound: 4 B written, 4 B read with
 * src_in). */
uint64_t dcc_select_alg_bytes(uint64_t n_txn, uint64_t n_sel, uint64_t nnz_sel,
                              int n_txn_arrays /* tn/order/src arrays carried */);

/* ------------------------------------ abort queue (back-off of the retries) */
/* The reference does not retry an aborted txn at once: WorkerThread bumps its
 * abort_cnt and hands it to AbortQueue::enqueue (system/worker_thread.cpp:
 * 165-168), which parks it until now + penalty(abort_cnt)
 * (system/abort_queue.cpp:26-50); AbortQueue::process releases the entries
 * with penalty_end < now in penalty_end order (:52-82, abort_queue.h:37-42).
 * This is that queue where the batch lives: the parked txns stay in device
 * memory, a push takes an epoch and its decisions, a pop writes the due txns
 * as the front of the next epoch's CSR.
 *
 * An entry is (due u64, seq u64, src u32, cnt u32, accesses).  seq is the push
 * ordinal over the queue's life; it is never stored: the pool is kept in seq
 * order.  The clock `now` is the caller's (ns, epochs, anything monotone);
 * nothing reads a real clock.
 *
 * Penalty, with cnt the abort count AFTER the increment (first abort: 1):
 *   DCC_BACKOFF_NONE       penalty                          (BACKOFF false)
 *   DCC_BACKOFF_REFERENCE  exactly what abort_queue.cpp:30 computes as C
 *                          parses it, in u64: max((penalty * 2) ^ cnt,
 *                          penalty_max) -- `^` is XOR and binds looser than
 *                          `*`, and it is max.  penalty 10, penalty_max 5,
 *                          cnt 1, 2, 3, 4, 5, 20: 21, 22, 23, 16, 17, 5.  With
 *                          the reference's defaults (config.h:112-114) it is
 *                          penalty_max for every realistic cnt.  The default.
 *   DCC_BACKOFF_EXP        the evident intent: min(penalty * 2^cnt,
 *                          penalty_max); penalty_max when cnt >= 64 or the
 *                          shift loses bits.
 * due = now + penalty(cnt), saturating at 2^64 - 1.
 *
 * Every buffer is allocated by dcc_abortq_create (both CSR pools, the per-txn
 * arrays, the sort buffers): a warmed-up push or pop of a device batch
 * allocates nothing.  The queue is always device-resident; on a
 * dcc_init_multi context it lives on rank 0's GPU.  No call is a collective.
 * Pipelined OCC epochs in flight complete first.  Work runs on the context's
 * stream.  A queue still alive at dcc_destroy is freed with its context. */
#define DCC_BACKOFF_REFERENCE 0
#define DCC_BACKOFF_NONE 1
#define DCC_BACKOFF_EXP 2
/* dcc_abortq_params.flags */
#define DCC_ABORTQ_SORT_FULL 0x1u /* pop sorts all 64 bits of `due` instead of only the bits
                                     that can differ among the due entries (A/B timing)       */
typedef struct dcc_abortq dcc_abortq;
typedef struct dcc_abortq_params {
  uint64_t cap_txn, cap_nnz; /* room, in parked txns / accesses; both < 2^32 */
  uint64_t penalty;          /* ABORT_PENALTY, in the caller's clock units   */
  uint64_t penalty_max;      /* ABORT_PENALTY_MAX                            */
  uint32_t policy;           /* DCC_BACKOFF_*                                */
  uint32_t flags;            /* DCC_ABORTQ_*                                 */
} dcc_abortq_params;
int dcc_abortq_create(dcc_ctx* ctx, const dcc_abortq_params* params, dcc_abortq** out);
void dcc_abortq_destroy(dcc_abortq* q);
/* Park the txns with rc[i] == want (the selection of dcc_batch_select: index
 * order, accesses in list order, empty txns kept, any txn length, any compact
 * batch form).  Entry: cnt = (cnt_in ? cnt_in[i] : 0) + 1, saturating at
 * 2^32 - 1; src = src_in ? src_in[i] : i; due from the penalty, computed on
 * the device.  rc / src_in / cnt_in live where the batch lives (device memory
 * with DCC_DEVICE_PTRS).  Malformed offsets give DCC_EINVAL.  More than the
 * queue's room, in txns or accesses, gives DCC_ERANGE: the queue is unchanged
 * and *out_n / *out_nnz (host memory, may be NULL) report what was needed;
 * otherwise they report what was parked.
 * Stats: n_commit = parked txns, n_abort = the rest, alg_bytes
 * (dcc_abortq_push_alg_bytes), device_ms, total_ms; with profiling phase_ms
 * as the select's. */
int dcc_abortq_push(dcc_abortq* q, const dcc_batch* batch, const uint8_t* rc, uint8_t want,
                    const uint32_t* src_in, const uint32_t* cnt_in, uint64_t now,
                    uint64_t* out_n, uint64_t* out_nnz, dcc_stats* out_stats);
/* Release every entry with due < now (strict, abort_queue.cpp:62), in
 * (due, seq) order, to rows out->txn_base.. / accesses out->nnz_base.. of
 * `out`, exactly as a select writes them (offsets[txn_base] = nnz_base is
 * written, the output is wide).  Their src goes to out->src; their cnt and
 * due to out_cnt / out_due, [txn_base + cap_txn] each, or NULL.  start_tn /
 * finish_tn / order of `out` are not written.  The other entries stay, in seq
 * order.  flags: DCC_DEVICE_PTRS when the arrays of `out`, out_cnt and
 * out_due are device memory; host memory otherwise.  A release that does not
 * fit cap_txn / cap_nnz, or whose nnz_base + accesses exceeds 2^32 - 1, gives
 * DCC_ERANGE: nothing is written, the queue is unchanged, *out_n / *out_nnz
 * report what was needed.  Nothing due gives DCC_OK, zero counts and
 * offsets[txn_base] = nnz_base.
 * Stats: n_commit = released txns, n_abort = left parked, alg_bytes
 * (dcc_abortq_pop_alg_bytes), device_ms, total_ms; with profiling phase_ms:
 * 0 = due flags and counts, 1 = sort, 2 = gather of the released txns,
 * 3 = compaction of the kept ones. */
int dcc_abortq_pop(dcc_abortq* q, uint64_t now, const dcc_select_out* out, uint32_t* out_cnt,
                   uint64_t* out_due, uint32_t flags, uint64_t* out_n, uint64_t* out_nnz,
                   dcc_stats* out_stats);
/* Parked txns / accesses: host state, no device work. */
int dcc_abortq_size(const dcc_abortq* q, uint64_t* out_n, uint64_t* out_nnz);
/* Drop every entry (the buffers stay). */
int dcc_abortq_clear(dcc_abortq* q);
/* Algorithmic bytes of a push: the select of the same txns with one per-txn
 * array (src) plus 12 per parked txn (cnt 4 B and due 8 B written):
 * dcc_select_alg_bytes(n_txn, n_sel, nnz_sel, 1) + 12 n_sel. */
uint64_t dcc_abortq_push_alg_bytes(uint64_t n_txn, uint64_t n_sel, uint64_t nnz_sel);
/* Algorithmic bytes of a pop of n_due txns / nnz_due accesses from a queue of
 * n_q / nnz_q: due and offsets of every entry read (8 n_q + 4(n_q+1)), one
 * (due, index) pair per entry written and read once (24 n_q; the radix
 * passes in between are not counted), every access moved once (18 nnz_q: the
 * released ones to `out`, the kept ones to the other pool), both offset
 * arrays written (4(n_due+1) + 4(n_q-n_due+1)), src / cnt / due of every
 * entry read and written (32 n_q).  Nothing due: the first term alone. */
uint64_t dcc_abortq_pop_alg_bytes(uint64_t n_q, uint64_t nnz_q, uint64_t n_due, uint64_t nnz_due);

/* Wave dispatch: the wave levels of an epoch
 * (out_wave of dcc_calvin_order_epoch) as the lists a dispatcher releases:
 * out_txn[out_wave_off[w] .. out_wave_off[w+1]) = the txns of wave w in
 * sequence order (order = the batch's sequencer key, NULL = index order;
 * ties keep index order).  Wave w+1 starts once every txn of wave w has
 * released its locks (TxnTable::restart_txn, txn_table.cpp:151-176, after the
 * lock_release promotions of row_lock.cpp:317-357).  *out_n_waves = max
 * wave + 1; out_wave_off needs *out_n_waves + 1 entries (off_cap; may be NULL
 * to query the count).  A wave level of 2^32-1 (the count would not fit) is
 * DCC_ERANGE.  Device pointers with DCC_DEVICE_PTRS in flags. */
int dcc_calvin_dispatch(dcc_ctx* ctx, const uint32_t* wave, const uint64_t* order, uint64_t n,
                        uint32_t flags, uint32_t* out_wave_off, uint64_t off_cap,
                        uint32_t* out_txn, uint32_t* out_n_waves);

/* ------------------------------------------------------------ GPU index */
/* The key -> row lookups execution does through IndexHash (index_insert /
 * index_read, storage/index_hash.cpp:58-137, 160-231) as one HBM table probed
 * for a whole epoch's accesses at once.  A key inserted more than once reads
 * as its newest insert (insert_item prepends, read_item takes the head); a
 * missing key (the reference's M_ASSERT_V, index_hash.cpp:221) reads as
 * DCC_ROW_NONE and is counted in *out_missing. */
#define DCC_ROW_NONE 0xFFFFFFFFFFFFFFFFull
/* keys / rows: host arrays.  A key equal to DCC_KEY_RESERVED rejects the
 * whole call with DCC_EINVAL before anything changes: none of its keys is
 * inserted and dcc_index_size stays. */
int dcc_index_insert(dcc_ctx* ctx, const uint64_t* keys, const uint64_t* rows, uint64_t n);
/* keys / out_rows: host arrays, or device arrays with DCC_DEVICE_PTRS in
 * flags.  DCC_KEY_RESERVED is never in the index: it reads as DCC_ROW_NONE
 * and counts as missing. */
int dcc_index_probe(dcc_ctx* ctx, const uint64_t* keys, uint64_t n, uint64_t* out_rows,
                    uint32_t flags, uint64_t* out_missing);
int dcc_index_clear(dcc_ctx* ctx);
uint64_t dcc_index_size(const dcc_ctx* ctx);      /* distinct keys            */
double dcc_index_last_ms(const dcc_ctx* ctx);     /* device ms of the last probe */

/* ----------------------------------------------------- batch producers */
/* Deterministic restatements of the reference workload generators
 * (SURVEY.md §8(a) a17/a18).  The reference seeds from the clock
 * (ycsb_query.cpp:31); here every chunk of `chunk_txns` transactions draws
 * from its own myrand stream (helper.cpp:144-147) seeded from `seed` and the
 * chunk index, so batches are reproducible and can be generated in parallel. */
typedef struct dcc_ycsb_params {
  uint64_t n_txn;
  uint32_t req_per_query;   /* REQ_PER_QUERY (config.h:177)                    */
  uint32_t part_cnt;        /* PART_CNT                                        */
  uint64_t table_size;      /* SYNTH_TABLE_SIZE (config.h:169)                 */
  double zipf_theta;        /* ZIPF_THETA                                      */
  double txn_write_perc;    /* TXN_WRITE_PERC                                  */
  double tup_write_perc;    /* TUP_WRITE_PERC                                  */
  uint32_t part_per_txn;    /* PART_PER_TXN (used with strict_ppt)             */
  uint32_t strict_ppt;      /* STRICT_PPT                                      */
  uint32_t first_part_local;/* FIRST_PART_LOCAL                                */
  uint32_t chunk_txns;      /* txns per generator stream; also the txns per
                               origin node for Calvin (home partition =
                               chunk index % part_cnt)                         */
  uint64_t seed;
  uint32_t n_threads;       /* host threads used to generate (0 = auto)        */
  uint32_t reserved;
} dcc_ycsb_params;
void dcc_ycsb_params_default(dcc_ycsb_params* p);
/* offsets [n_txn+1], keys/acctype [n_txn*req_per_query]; home may be NULL. */
int dcc_gen_ycsb(const dcc_ycsb_params* p, uint32_t* offsets, uint64_t* keys,
                 uint8_t* acctype, uint32_t* home);

typedef struct dcc_tpcc_params {
  uint64_t n_txn;
  uint32_t num_wh;          /* NUM_WH                                          */
  uint32_t part_cnt;        /* PART_CNT (wh_to_part, tpcc_helper.cpp:161-164)  */
  double perc_payment;      /* PERC_PAYMENT                                    */
  uint32_t wh_update;       /* WH_UPDATE (config.h:194)                        */
  uint32_t max_items;       /* MAX_ITEMS_NORM (config.h:187)                   */
  uint32_t cust_per_dist;   /* CUST_PER_DIST_NORM (config.h:188)               */
  uint32_t dist_per_wh;     /* DIST_PER_WH (config.h:223)                      */
  uint32_t max_items_per_txn; /* MAX_ITEMS_PER_TXN (config.h:189)              */
  uint32_t part_per_txn;
  double mpr;               /* MPR                                             */
  uint32_t first_part_local;
  uint32_t chunk_txns;
  uint64_t seed;
  uint32_t n_threads;
  uint32_t reserved;
} dcc_tpcc_params;
void dcc_tpcc_params_default(dcc_tpcc_params* p);
/* Upper bound of accesses per TPC-C txn (NewOrder: 3 + 2*MAX_ITEMS_PER_TXN). */
uint32_t dcc_tpcc_max_access(const dcc_tpcc_params* p);
/* offsets [n_txn+1]; keys/acctype sized n_txn*dcc_tpcc_max_access(p);
 * txn_type [n_txn] (TPCCTxnType: 1 = PAYMENT, 2 = NEW_ORDER) may be NULL. */
int dcc_gen_tpcc(const dcc_tpcc_params* p, uint32_t* offsets, uint64_t* keys,
                 uint8_t* acctype, uint8_t* txn_type, uint64_t* out_nnz);

/* Canonical TPC-C key: (table_id << 56) | index key. */
#define DCC_TPCC_KEY(table_id, ikey) ((((uint64_t)(table_id)) << 56) | ((uint64_t)(ikey)))

/* ------------------------------------------------- batch files (.dccb) */
/* One captured epoch on disk: the CSR access lists,
 * optional timestamps / sequencer order, optional decisions.  Versioned,
 * checksummed (FNV-1a 64), little-endian; layout in batch_file.cpp.  Host
 * pointers only.  Version 2's checksum also covers the header fields. */
#define DCC_FILE_VERSION 2   /* written; version 1 files are still read */
#define DCC_FILE_OCC 1
#define DCC_FILE_CALVIN 2
#define DCC_FILE_HAS_TN 0x1u         /* start_tn + finish_tn                     */
#define DCC_FILE_HAS_ORDER 0x2u      /* Calvin sequencer order                   */
#define DCC_FILE_HAS_RC 0x4u         /* per-txn RC                               */
#define DCC_FILE_HAS_COMMIT_TN 0x8u  /* OCC history tn of committed writers      */
#define DCC_FILE_HAS_GROUP 0x10u     /* Calvin grant group per request           */
#define DCC_FILE_HAS_WAVE 0x20u      /* Calvin wave per txn                      */
typedef struct dcc_file_info {
  uint32_t version;     /* DCC_FILE_VERSION                                      */
  uint32_t kind;        /* DCC_FILE_OCC / DCC_FILE_CALVIN                        */
  uint32_t sections;    /* DCC_FILE_HAS_* bits present (read); ignored on write  */
  uint32_t reserved;
  uint64_t n_txn, nnz;  /* read only (taken from the batch on write)             */
  uint64_t seed;        /* generator seed or capture id                          */
  uint64_t epoch;       /* epoch number within a capture                         */
  uint64_t tnc_before;  /* OCC commit counter before the epoch (occ.h:67)        */
} dcc_file_info;
/* Sections are written for every non-NULL array (start_tn/finish_tn/order from
 * the batch).  Returns DCC_EIO on a file error. */
int dcc_file_write(const char* path, const dcc_file_info* info, const dcc_batch* batch,
                   const uint8_t* rc, const uint64_t* commit_tn, const uint32_t* group,
                   const uint32_t* wave);
int dcc_file_read_info(const char* path, dcc_file_info* info);
/* Fills every non-NULL destination whose section is present (size them from
 * dcc_file_read_info).  DCC_EINVAL: bad magic, truncated, checksum or offsets
 * mismatch; DCC_ENOTSUP: another format version. */
int dcc_file_read(const char* path, uint32_t* offsets, uint64_t* keys, uint8_t* acctype,
                  uint64_t* start_tn, uint64_t* finish_tn, uint64_t* order, uint8_t* rc,
                  uint64_t* commit_tn, uint32_t* group, uint32_t* wave);

/* Algorithmic bytes of one epoch pass:
 * 4(N+1) + 9 nnz + 16 nnz_w + 16 nnz + N. */
uint64_t dcc_alg_bytes(uint64_t n_txn, uint64_t nnz, uint64_t nnz_w);
/* Algorithmic bytes of one Calvin epoch: 4(N+1) offsets + 9 nnz (key, type)
 * + 4 nnz (grant group) + N (RC) [+ 8N order] [+ 4N wave]. */
uint64_t dcc_calvin_alg_bytes(uint64_t n_txn, uint64_t nnz, int with_order, int with_wave);

#ifdef __cplusplus
}
#endif
#endif /* DCC_H_ */
