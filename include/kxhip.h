/* kxhip.h — C ABI of the MI355X streaming-SST engine (libkxhip.so).
 *
 * This is the drop-in boundary for the reference's run-time hot path.  In the
 * reference the generated code talks to its runtime through the "program
 * interface" of crt/crt.c:101-105 (`init`, `match(phase)`) and the runtime
 * exports readnext/consume/outputconst/outputarray/output/append/appendarray/
 * concat/reset (crt/crt.c:107-324); the whole thing is driven by `main`/`run`
 * (crt/crt.c:356-467).  Here the seam sits one level up: a compiled program
 * (KXP blob, include/kxp_format.h — the table form of the IL `Pipeline`,
 * src/KMC/Program/IL.hs:69-90) is handed to an engine that owns the state
 * loop, the registers and the output buffer on the GPU.
 *
 *   reference                                   this ABI
 *   ---------                                   --------
 *   compileProgram … Pipeline (C.hs:529-540)    kx_load(blob)
 *   run(phase): init_outbuf, init, match,       kx_run_device / kx_run_host /
 *     flush_outbuf        (crt.c:356-364)         kx_run_fd
 *   main: -t timing, phase pipeline             kx_run_fd + kx_stats (kxrun.cpp
 *     (crt.c:372-467)                             is the `main`)
 *   fail<K>: "Match error at input symbol %zu"  return 1, stats->fail_pos
 *     exit(1)             (C.hs:79-81)
 *
 * Plain pointers and sizes only; no framework types.  Device pointers are HIP
 * device pointers on the current device; `stream` is a hipStream_t (NULL =
 * default stream).  One kx_program may be used by one host thread at a time.
 *
 * Return codes: 0 accepted; 1 match error (stats->fail_pos = number of input
 * symbols consumed before the failing state, stats->fail_stage = pipeline
 * stage; no output is produced — the reference itself loses the un-flushed
 * tail, crt/crt.c:217-227); <0 runtime error, message in kx_last_error().
 */
#ifndef KXHIP_H
#define KXHIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct kx_program kx_program;
typedef struct kx_shard kx_shard;

#define KX_OK 0
#define KX_MATCH_ERROR 1
#define KX_E_BLOB (-1)     /* malformed / unsupported program blob          */
#define KX_E_HIP (-2)      /* HIP runtime error                             */
#define KX_E_CAPACITY (-3) /* output buffer too small; *out_len = needed    */
#define KX_E_ARG (-4)
#define KX_E_IO (-5)

enum { KX_K_SYNC = 0, KX_K_FORWARD = 1, KX_K_HEAD = 2, KX_K_BACKLEN = 3, KX_K_RESOLVE = 4, KX_K_EMIT = 5, KX_NKERNELS = 6 };

typedef struct kx_stats {
  uint64_t fail_pos;            /* valid when the call returned 1                           */
  uint32_t fail_stage;
  uint32_t unsynced_segments;   /* segments whose start state had to be chained sequentially */
  uint64_t in_bytes, out_bytes;
  float kernel_ms[KX_NKERNELS]; /* HIP-event time of each kernel group, summed over the stages  */
  float total_ms;               /* first launch → last kernel done, all stages               */
  uint32_t emit_overflow_pieces; /* output stage: pieces that needed a second sweep (last stage run) */
} kx_stats;

/* tuning knobs (0 = default, in every field).  Round 6: what used to be environment variables of the library (KX_DF, KX_DF_K, KX_INL,
 * KX_JL, KX_EMIT_*, KX_NO_*, KX_FORCE_*, KX_ACT_*, KX_DEBUG_FLAGS) is here; the library itself reads only KX_DEBUG (chatter on stderr),
 * KX_FD_TRACE, KX_WINDOW_BYTES and KX_READ_THREADS (kx_run_fd's host side).  The produced binary (kxrun.cpp) and the Python test
 * binding (kleenexlang_amd/host.py) map the old variable names onto this struct, so scripts keep working.
 * LOAD-TIME fields decide how the tables are built: they take effect in kx_load_config; kx_set_config refuses to change them. */
typedef struct kx_config {
  uint32_t segment_bytes;  /* input bytes per lane; multiple of 64; 0 = one round of lanes (4-64 KiB)  */
  uint32_t block_threads;  /* workgroup size (power of two); default 512        */
  uint32_t collect_timing; /* record per-kernel HIP events into kx_stats        */
  uint32_t phase;          /* kx_run_fd: 0 = the whole pipeline; K = only phase K, stdin -> stdout (`BIN --phase K`, crt/crt.c:390-393,408-411) */
  uint64_t window_bytes;   /* kx_run_fd: input bytes resident at a time; 0 = 1 GiB (env KX_WINDOW_BYTES overrides;
                              KX_READ_THREADS = pread threads per chunk of a regular file, default 4; KX_FD_TRACE=1 prints where
                              the reader / compute / writer threads spent their time) */
  /* ---- which engine (load time) ---- */
  uint32_t delayed_form;   /* 0 auto (taken where at most a quarter of the start-reachable transitions are undecided), 1 never,
                              2 whatever that share                                                          [KX_DF=0 / 2] */
  uint32_t delay;          /* 0 auto (1 where one symbol decides everything the start state reaches, else 2), 1, 2   [KX_DF_K] */
  uint32_t merge_window;   /* merged constants (kx_delayed.h): 0 auto (the largest J <= 8 whose table image leaves k_dforward two
                              blocks per CU), else J = merge_window - 1 (1: none)                                   [KX_DF_J = J] */
  uint32_t inline_consts;  /* general engine, inline-constant entry layout: 0 auto, 1 off, 2 on                    [KX_INL=0 / 1] */
  uint32_t job_stride;     /* general engine, job-stride entry layout: 0 auto (a second image, chosen shard by shard from the
                              constants per piece), 1 off, 2 on (only that image)                [KX_JL_AUTO_OFF / KX_JL=0 / 1] */
  uint32_t disable;        /* KX_OFF_* bits                                                                             */
  uint32_t force;          /* KX_FORCE_* bits                                                                           */
  /* ---- the output stage's plan (run time) ---- */
  uint32_t emit_waves;     /* waves per CU of k_emit / k_demit: 0 auto (12), 4, 8, 12, 16 (16: delayed form only)   [KX_EMIT_WAVES] */
  uint32_t emit_half;      /* k_demit, a lane takes half a piece: 0 auto (where 64 pieces outgrow a wave's staging), 1 off, 2 on [KX_EMIT_HALF] */
  uint32_t emit_inplace;   /* k_emit, constants copied by the sweeping lane instead of jobs: 0 auto, 1 off, 2 on    [KX_EMIT_INPLACE] */
  uint32_t emit_staging;   /* k_emit, staging bytes per wave: 0 auto                                                 [KX_EMIT_STG] */
  uint32_t df_backoff;     /* after a shard left the delayed form: 0 = the stage skips 2^k - 1 shards after the k-th fall-back in a
                              row (at most 63), 1 = every shard tries the form again                                        */
  uint32_t debug_flags;    /* 64: per-phase shader-clock timeline of k_emit / k_demit (printed under KX_DEBUG)     [KX_DEBUG_FLAGS] */
  /* ---- the action post-pass (run time) ---- */
  uint32_t act_par_min;    /* bytes from which a token stream is replayed chunk-parallel: 0 = 1 MiB                 [KX_ACT_PAR_MIN] */
  uint32_t act_prefix3_min;/* blocks from which the safe-point prefix runs in three steps: 0 = 65536             [KX_ACT_PREFIX3_MIN] */
  uint32_t act_lanes;      /* one lane per chunk (token-dense streams): 0 auto, 1 off, 2 on                           [KX_ACT_LANES] */
  uint32_t act_chunk;      /* wanted chunk bytes: 0 auto (2048 / 4096)                                                 [KX_ACT_CHUNK] */
  /* ---- batched runs (run time) ---- */
  uint32_t batch_actions;  /* kx_run_batch, stages with register actions: 0 / 1 = every document takes the single-document route,
                              2 = the batch replay (k_bact_*: one lane or one wave per document)          [KX_BATCH_ACTIONS=0 / 1] */
  uint32_t batch_doc_max;  /* kx_run_batch: longest document the batch kernels take; longer ones go through the single-document
                              route: 0 = 64 KiB                                                                                */
  uint32_t reserved[3];    /* must be 0 */
} kx_config;
#define KX_OFF_DIRECT 1u     /* load: entries of the plain layout name their action, not the constant's pool slot    [KX_NO_DIRECT] */
#define KX_OFF_PAIR 2u       /* load: no two-symbol table for k_forward                                                 [KX_NO_PAIR] */
#define KX_OFF_CMPX 4u       /* load: constants of at most 16 bytes are not stored by the v_cmpx sequences              [KX_NO_CMPX] */
#define KX_OFF_COOP 8u       /* run:  k_forward without cooperative line loads                                          [KX_NO_COOP] */
#define KX_OFF_SLOW 16u      /* load: no exact slow path in the delayed form's forward pass: a context that the delay does not decide
                                sends the whole shard to the general engine, as in round 5                              [KX_NO_SLOW] */
#define KX_FORCE_BIG 1u      /* load: tables stay in global memory whatever their size (the BIG instances; tests)     [KX_FORCE_BIG] */
#define KX_FORCE_TBLMODE 2u  /* load: per-entry symbol-table ids even where one table would do (tests)            [KX_FORCE_TBLMODE] */
#define KX_FORCE_ACT_SEQ 4u  /* run:  the action post-pass on one wave                                                  [KX_ACT_SEQ] */
#define KX_FORCE_SAME_DEVICE 8u /* kx_run_fd_sharded_cfg: every rank on the caller's current device (a one-GPU box)  [KX_SHARD_SAME_DEVICE] */

int kx_load(const void* blob, size_t blob_len, kx_program** prog);   /* = kx_load_config(blob, blob_len, NULL, prog) */
/* kx_load with the load-time fields of `cfg` (NULL: all defaults); its run-time fields become the program's configuration. */
int kx_load_config(const void* blob, size_t blob_len, const kx_config* cfg, kx_program** prog);
/* Structural check of a blob without touching a device: every section inside the blob, every index inside its table,
 * the engine's size limits.  0 or KX_E_BLOB (kx_load performs the same checks). */
int kx_validate(const void* blob, size_t blob_len);
void kx_free(kx_program* prog);
const char* kx_last_error(void);
int kx_set_config(kx_program* prog, const kx_config* cfg);   /* run-time fields; KX_E_ARG if a load-time field differs from what the program was loaded with */
uint32_t kx_num_stages(const kx_program* prog);
/* 1: the stage uses register actions (`r@t`, `!r`, `[r <- …]`).  Its transducer output is a token stream (kxp_format.h) that
 * kx_run_device / kx_run_host / kx_run_fd replay with the action post-pass before it leaves the stage; the replay is
 * sequential over the whole stream (registers are unbounded), so such a stage is not run through the kx_shard_* protocol
 * across GPUs (SURVEY §8e "pathological case": the boundary tuple would be O(N)). */
int kx_stage_has_actions(const kx_program* prog, uint32_t stage);

/* ---- the delayed form of a stage (round 5; kleenexlang_amd/csrc/engine/kx_delayed.h) -----------------------------------
 * Where every step's output is decided by at most K further input symbols the engine runs the stage as a forward transducer
 * with fixed delay K — a forward pass for the lengths and one fused walk that places the bytes; no backward pass.  A context
 * that K symbols do not decide is noticed at run time and the shard is redone by the general engine (and the stage backs off
 * from the form for a while): results never depend on which engine ran.  kx_config::delayed_form / delay / merge_window select it.
 * kx_df_describe needs no device: it builds the form from the blob (as kx_load does; the `_cfg` variants with the load-time fields of a
 * configuration, the plain ones with the defaults) and reports it; `image`, if not NULL,
 * receives up to image_cap bytes of the table image (class*8 u8[256] — the class index where a stage has more than 31 byte classes — | rows of C x {lo = handle of the next state's row,
 * hi = what the step writes: bit 0 no byte copied, bits 10-22 pool offset/16 of the constant, bit 23 a constant follows,
 * bits 24-30 bytes appended} | pool).  kx_df_pending: what slot j (0 = oldest) of product state `state` still owes, per leaf
 * of its SST state: copy | path-constant id << 1 (n_out = 1: the same for every leaf) — the host evaluates these at the end
 * leaf to write a shard's last K steps.  Returns 0, KX_E_BLOB, or KX_E_ARG (no such stage / state / slot). */
typedef struct kx_df_info {
  uint32_t available;      /* 1: the stage has a delayed form and the engine takes it */
  uint32_t delay;          /* K */
  uint32_t nstates;        /* product states (the dead and the escape row follow them in the image) */
  uint32_t nclasses;
  uint32_t image_bytes, off_pool, start_handle, dead_handle, escape_handle;
  uint32_t transitions, escapes;               /* over the whole table */
  uint32_t transitions_start, escapes_start;   /* over the part reachable from the program's start state */
  uint32_t merge_window;   /* J: steps a constant may wait to be written together with the next one (0: no merged constants) */
  char reason[96];         /* why not, if available == 0 */
} kx_df_info;
int kx_df_describe(const void* blob, size_t blob_len, uint32_t stage, kx_df_info* info, void* image, size_t image_cap);
int kx_df_pending(const void* blob, size_t blob_len, uint32_t stage, uint32_t state, uint32_t slot, uint32_t* sst_state,
                  uint32_t* kinds, uint32_t* n_out);
int kx_df_describe_cfg(const void* blob, size_t blob_len, uint32_t stage, const kx_config* cfg, kx_df_info* info, void* image, size_t image_cap);
int kx_df_pending_cfg(const void* blob, size_t blob_len, uint32_t stage, const kx_config* cfg, uint32_t state, uint32_t slot,
                      uint32_t* sst_state, uint32_t* kinds, uint32_t* n_out);
/* Merged constants (round 6): a constant may wait up to J = merge_window steps for the next one as long as no copied byte can come
 * between them, so that one job of the output stage places both (apache_log: 15 constants per line become 8).  A product state then
 * also holds the constants that are DUE; kx_df_deferred returns their bytes, oldest first (a shard's tail writes them in front of
 * what the pending steps append).  *n_out = their length (which may exceed cap; at most cap bytes are stored). */
int kx_df_deferred(const void* blob, size_t blob_len, uint32_t stage, const kx_config* cfg, uint32_t state, void* bytes, size_t cap, size_t* n_out);
/* The handle of (SST state q, nothing pending, nothing due): where a segment, a window or a shard may begin.  *handle = 0xFFFF where
 * the table does not hold it (the part reachable from the start state never visits q). */
int kx_df_start_of_state(const void* blob, size_t blob_len, uint32_t stage, const kx_config* cfg, uint32_t sst_state, uint32_t* handle);
/* of a loaded program: 0 the stage has no delayed form, 1 its next shard runs on it, 2 a shard gave it up (escape) and the stage is backing
 * off: after the k-th fall-back in a row the next 2^k - 1 shards (at most 63) go straight to the general engine, then the form is tried again
 * (kx_config::df_backoff = 1: at once); 3 a shard left the form in (nearly) every segment (at least one lane in 16, and 8 lanes): the
 * program's output hangs on unbounded lookahead and the stage stays on the general engine until kx_stage_reset_delayed_form */
int kx_stage_delayed_form(const kx_program* prog, uint32_t stage);
/* forget the back-off: the stage's next shard tries the delayed form again (no-op for a stage without one) */
void kx_stage_reset_delayed_form(kx_program* prog, uint32_t stage);

/* ---- what the loader builds for a stage (kleenexlang_amd/csrc/engine/kx_stage.h) --------------------------------------------
 * kx_stage_describe_cfg needs no device: it runs the host-only stage builder as kx_load_config does (cfg NULL: all defaults) and
 * reports the layout it decided, the scalar fields of the structs the kernels take, and the bytes of one of the stage's device
 * allocations.  Every pointer field of those structs appears as its byte offset into the allocation it points into.  `image`, if
 * not NULL, receives up to image_cap bytes of allocation `which`; info->image_bytes is its size (0: the stage has none, e.g. no
 * job-stride alternative).  Set info->size = sizeof(kx_stage_info) before the call.  Returns 0, KX_E_BLOB or KX_E_ARG. */
#define KX_STAGE_MAIN 0u     /* the general engine's tables (info->t describes them)                                         */
#define KX_STAGE_ALT 1u      /* the same stage in the job-stride layout, where kx_load_config keeps both (info->t describes IT) */
#define KX_STAGE_DELAYED 2u  /* the delayed form's table image | start_of_state                                              */
#define KX_STAGE_SLOW 3u     /* the tables of the delayed form's exact slow path                                             */
typedef struct kx_stage_info {
  uint32_t size;           /* sizeof(kx_stage_info) */
  uint32_t which;
  uint64_t image_bytes;
  uint32_t general, big, has_alt, has_df, actions, action_regs, max_const_len, reserved0;
  uint64_t lds_bytes, sync_lds_bytes;
  struct {                 /* the general engine's DevTables; packed … init_len: offsets into KX_STAGE_MAIN / KX_STAGE_ALT */
    uint64_t packed, pair, wlen, cls, nleaves, fin_leaf, sync16, init_off, init_len;
    uint32_t packed_words, off_fwd, off_ent, off_pool, off_cls, off_adesc, naid, nstates, nclasses, q0h, maxleaves, deadh, nullrow, cshift,
        debug, big, hshift, rshift, rbase, stage_words, pair_words, pair_magic, nsync, sync_multi, sync_words, off_tbl, xlat, tblmode,
        aid_mask, inl, jl, direct, short_consts, reserved0;
  } t;
  struct {                 /* the delayed form's DfDev (all zero without one); img, start_of_state: offsets into KX_STAGE_DELAYED;
                              sl_nleaves, sl_fin_leaf, sl_cls: into KX_STAGE_MAIN; the other sl_*: into KX_STAGE_SLOW */
    uint64_t img, start_of_state, sl_fmap, sl_back, sl_nleaves, sl_fin_leaf, sl_cls, sl_pcoff, sl_pcpool, sl_pend, sl_defoff, sl_defpc, sl_q;
    uint32_t words, off_pool, deadh, esch, starth, K, C, orig_c4, hshift, short_consts, debug, nstates, J, wide, sl_Lm, sl_npc, sl_on, reserved0;
  } d;
} kx_stage_info;
int kx_stage_describe_cfg(const void* blob, size_t blob_len, uint32_t stage, const kx_config* cfg, uint32_t which, kx_stage_info* info,
                          void* image, size_t image_cap);

/* Whole program (all pipeline stages) over one device-resident input.
 * d_out may be NULL with cap 0 to query the exact output size (returned in
 * *out_len with KX_E_CAPACITY).  Blocks until the result is complete.
 * What the call writes and reads (tests/test_run_device_gpu.py holds it to this):
 *   - d_out is 16-byte aligned, KX_E_ARG otherwise, before anything is launched.  (A program whose last stage has register actions
 *     copies its result bytewise and takes any address.)
 *   - Nothing outside d_out[0, *out_len) is written, whatever `cap` says: room beyond the result is not scratch space.
 *   - On KX_MATCH_ERROR, KX_E_CAPACITY and KX_E_ARG d_out is untouched.
 *   - d_in may have any alignment (an address that is not 16-byte aligned costs a copy of the input), is never written, and no byte
 *     outside d_in[0, n) influences the result.
 *   - All device work is queued on `stream` (NULL: the default stream), behind whatever the caller has queued there. */
int kx_run_device(kx_program* prog, const void* d_in, size_t n, void* d_out, size_t cap, size_t* out_len,
                  kx_stats* stats, void* stream);

/* Host-buffer convenience: H2D, run, D2H.  *out is malloc'd (free with kx_host_free). */
int kx_run_host(kx_program* prog, const void* in, size_t n, void** out, size_t* out_len, kx_stats* stats);
void kx_host_free(void* p);

/* stdin → stdout contract of the produced binary (crt/crt.c:294-312,107-136): reads in_fd to EOF,
 * writes the output to out_fd. */
int kx_run_fd(kx_program* prog, int in_fd, int out_fd, kx_stats* stats);

/* ---- batched runs: many independent documents in one call ------------------------------------------------------------
 * A batch is n_docs documents; document i is the bytes d_in[d_in_off[i], d_in_off[i+1]).  d_in_off holds n_docs + 1
 * non-decreasing offsets (d_in_off[0] need not be 0: a slice of a larger buffer is a batch; documents may start at any byte
 * alignment; empty documents are allowed).  Every document is a whole input — it starts in the initial state, must end in a
 * final state, and every pipeline stage runs on it — and its result is, byte for byte, what kx_run_device gives for that
 * document alone.  All arrays live on the device; the call blocks until the result is complete.
 *   accepted document i: its output is d_out[d_out_off[i], d_out_off[i+1]) (d_out_off: n_docs + 1 entries, an exclusive
 *     prefix sum, d_out_off[0] = 0); d_docs[i] = {0, 0, 0}
 *   rejected document i: its output range is empty; d_docs[i] = {fail_pos, 1, fail_stage}, fail_pos being the number
 *     kx_run_device reports for the document alone.  Later stages do not run it.  Its neighbours' results do not change.
 * Return codes — NOTE: 1 does not mean "no output" here, unlike kx_run_device:
 *   0  every document was accepted
 *   1  at least one document was rejected; the outputs of the accepted documents are complete
 *   KX_E_CAPACITY  *out_len = the bytes needed; d_out_off and d_docs are filled.  d_out = NULL, cap = 0 is the size query.
 *   KX_E_ARG  among others: the offsets decrease somewhere (checked on the device before anything reads a document)
 *   < 0  other errors, as elsewhere (kx_last_error)
 * The batch kernels take documents of at most kx_config::batch_doc_max bytes, one lane per document.  Longer documents go
 * through the single-document driver one at a time (stats->docs_routed counts them).  A stage with register actions
 * (kx_stage_has_actions) emits a token stream per document, which has to be replayed: with kx_config::batch_actions = 2 the
 * batch kernels do it, one lane or one wave per document (stats->docs_replayed), and only a document longer than
 * batch_doc_max, or one whose replay outgrows its per-document arena, takes the route.  With batch_actions = 0 or 1 (the
 * library's default) EVERY document of such a stage takes the route: correct, but ~0.35 ms per document.  A call leaves
 * kx_stage_delayed_form of every stage as it found it. */
typedef struct kx_batch_doc {
  uint64_t fail_pos;
  uint32_t status;      /* 0 accepted, 1 match error */
  uint32_t fail_stage;
} kx_batch_doc;
typedef struct kx_batch_stats {
  uint64_t docs, docs_rejected;
  uint64_t docs_routed;    /* document runs that took the single-document route, summed over the stages */
  uint64_t in_bytes, out_bytes;
  float forward_ms, back_ms, scan_ms, emit_ms, routed_ms, total_ms;   /* HIP events, with kx_config::collect_timing; summed over the stages */
  uint64_t docs_replayed;  /* document runs of action stages replayed by the batch kernels (kx_config::batch_actions = 2), summed over the stages */
  float actions_ms;        /* the batch replay: measure + both replay kernels (HIP events, as above) */
  uint32_t reserved[1];
} kx_batch_stats;
int kx_run_batch(kx_program* prog, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, void* d_out, size_t cap,
                 uint64_t* d_out_off, kx_batch_doc* d_docs, size_t* out_len, kx_batch_stats* stats, void* stream);

/* ---- framed batches: documents that end before the next one starts, outputs that end in a terminator ---------------------------
 * kx_run_batch with a frame.  Document i is d_in[d_in_off[i], d_in_off[i+1] - trim): the last `trim` bytes of every range (a
 * record separator, say) belong to no document; with last_whole != 0 document n_docs - 1 is not trimmed (a last record without a
 * separator).  The trim applies to the input of stage 0 only.  The suffix[0, suffix_len) bytes follow the output of every ACCEPTED
 * document — one whose output is empty included — inside its range of d_out_off; a rejected document's range stays empty.  The
 * suffix is added behind the last stage only.  Everything else is kx_run_batch: a document's result (output, fail_pos) is what
 * kx_run_device gives for the trimmed document alone; *out_len, KX_E_CAPACITY, the size query and stats->out_bytes count the
 * suffixes.  frame == NULL or an all-zero frame IS kx_run_batch, bit for bit.
 * KX_E_ARG besides kx_run_batch's: a trimmed range shorter than `trim` (found on the device, with the decreasing offsets, before
 * any kernel reads a document), suffix_len > 8, a non-zero reserved word. */
typedef struct kx_batch_frame {
  uint32_t trim;         /* bytes cut from the end of every document's range                       */
  uint32_t last_whole;   /* != 0: the last document keeps its whole range                          */
  uint32_t suffix_len;   /* 0 to 8                                                                 */
  uint8_t suffix[8];
  uint32_t reserved[3];  /* must be 0 */
} kx_batch_frame;
int kx_run_batch_framed(kx_program* prog, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_frame* frame,
                        void* d_out, size_t cap, uint64_t* d_out_off, kx_batch_doc* d_docs, size_t* out_len, kx_batch_stats* stats,
                        void* stream);

/* ---- record mode: every separator-terminated record of a stream as its own input ----------------------------------------
 * A record is the bytes up to and including a separator byte; a non-empty tail after the last separator is a last record;
 * empty input has no records.  Each record's result is what kx_run_device gives for it alone (every stage runs). */
/* offsets of the records of d_in[0, n) split after every `sep` byte (a non-empty tail is a last record):
   d_off[0] = base, d_off[i] = base + end of record i, d_off[*n_records] = base + n.  cap < *n_records + 1:
   KX_E_CAPACITY with *n_records set (d_off = NULL, cap = 0 is the size query).  Device pointers; blocks. */
int kx_split_records(const void* d_in, size_t n, uint8_t sep, uint64_t base, uint64_t* d_off, uint64_t cap,
                     uint64_t* n_records, void* stream);

typedef struct kx_records_stats {
  uint64_t records, records_rejected, records_routed, in_bytes, out_bytes, windows, longest_record;
  float split_ms, batch_ms, total_ms;   /* split_ms, batch_ms: HIP events with kx_config::collect_timing; total_ms: wall time */
  uint32_t reserved[4];
} kx_records_stats;
/* the stream on in_fd in record mode: the outputs of the accepted records, in input order, to out_fd; one line
   "Match error at input symbol S in record R!" per rejected record to report_fd (-1: none), S the record's own fail_pos,
   R counted from 1.  Returns 0 (every record accepted), KX_MATCH_ERROR (some rejected; the rest is written in full) or an
   error.  Windows as kx_run_fd (kx_config::window_bytes, KX_WINDOW_BYTES); kx_config::phase must be 0.  Records of a stage
   with register actions are replayed by kx_run_batch's batch kernels where kx_config::batch_actions = 2 (the produced binary
   sets it for --records); otherwise each takes the single-document route (records_routed): correct, not fast. */
int kx_run_records_fd(kx_program* p, int in_fd, int out_fd, uint8_t sep, int report_fd, kx_records_stats* stats);

/* ---- quote-aware record mode: a separator inside quotes ends no record ----------------------------------------------------
 * The quote state at a byte is the parity of the `quote` bytes before it, from the start of the stream (parity_in carries it
 * into a buffer); a `sep` byte ends a record only at even parity.  A doubled quote ("" inside a quoted field) toggles twice, so
 * RFC 4180 splits right with no escape rule; every record boundary has even parity.  A stray unbalanced quote inverts the
 * state for the rest of the stream (with no quote after it, the rest is one record).  Backslash escapes are not understood
 * here: kx_split_records_escaped / kx_run_records_fd_escaped below add them.  quote == sep is KX_E_ARG. */
/* kx_split_records for d_in[0, n) with quote byte `quote` and the parity at d_in[0] parity_in (0 or 1, else KX_E_ARG).  Offsets,
   capacity and size query as kx_split_records; *parity_out (may be NULL) = parity_in ^ (quotes in the buffer & 1). */
int kx_split_records_quoted(const void* d_in, size_t n, uint8_t sep, uint8_t quote, uint32_t parity_in, uint64_t base,
                            uint64_t* d_off, uint64_t cap, uint64_t* n_records, uint32_t* parity_out, void* stream);
/* kx_run_records_fd with the quoted split; the parity carries from window to window (it starts at 0). */
int kx_run_records_fd_quoted(kx_program* p, int in_fd, int out_fd, uint8_t sep, uint8_t quote, int report_fd,
                             kx_records_stats* stats);

/* ---- escape-aware record mode: an escaped byte is only data ----------------------------------------------------------------
 * An unescaped `escape` byte E escapes the next byte; an escaped byte is never a separator, a quote or an escape (so E E is a
 * literal E, and the byte after it is live again).  Escapes apply inside and outside quotes; nothing is stripped.  `quote` is a
 * byte value or -1 (no quotes); with one, a separator ends a record only if it is unescaped and at even parity of the unescaped
 * quotes before it.  The state at a byte: bit 0 the quote parity (0 without a quote), bit 1 the byte is escaped; state_in gives
 * it at d_in[0] and carries it into a buffer.  escape == sep, escape == quote, quote == sep, quote outside [-1, 255], state_in > 3
 * or bit 0 of state_in without a quote are KX_E_ARG. */
/* kx_split_records for d_in[0, n) with the escape byte `escape`, the quote byte `quote` (-1: none) and the state at d_in[0]
   state_in.  Offsets, capacity and size query as kx_split_records; *state_out (may be NULL) = the state after the last byte. */
int kx_split_records_escaped(const void* d_in, size_t n, uint8_t sep, int quote, uint8_t escape, uint32_t state_in, uint64_t base,
                             uint64_t* d_off, uint64_t cap, uint64_t* n_records, uint32_t* state_out, void* stream);
/* kx_run_records_fd with the escaped split; the state carries from window to window (it starts at 0). */
int kx_run_records_fd_escaped(kx_program* p, int in_fd, int out_fd, uint8_t sep, int quote, uint8_t escape, int report_fd,
                              kx_records_stats* stats);

/* ---- record mode with a multi-byte separator ----------------------------------------------------------------------------------
 * The separator rs is 1 to 8 bytes.  Records end after the leftmost, non-overlapping copies of rs, found left to right (the
 * boundaries of Python's data.split(rs)): in "\n\n\n\n\n" with rs = "\n\n" only every second candidate counts.  The separator
 * stays in the record, nothing is stripped, a non-empty tail is a last record.  A buffer is split with a context: the last
 * min(rs_len - 1, length of the unfinished record so far) bytes before it, all of which belong to the unfinished record, so that
 * a separator may straddle two buffers.  With rs_len = 1 the offsets are kx_split_records's. */
/* kx_split_records for d_in[0, n) with the separator rs[0, rs_len) and the context ctx_in[0, ctx_in_len) (host pointers).
   Offsets, capacity and size query as kx_split_records.  On success (return 0) ctx_out[0, *ctx_out_len) (host, room for 7
   bytes) is the context for the buffer that follows, and *tail_len the bytes of this buffer behind its last selected separator:
   its last record is complete iff *tail_len == 0.  ctx_out, ctx_out_len and tail_len may be NULL.  rs_len outside 1..8 or
   ctx_in_len >= rs_len is KX_E_ARG. */
int kx_split_records_rs(const void* d_in, size_t n, const uint8_t* rs, uint32_t rs_len, const uint8_t* ctx_in, uint32_t ctx_in_len,
                        uint64_t base, uint64_t* d_off, uint64_t cap, uint64_t* n_records, uint8_t* ctx_out, uint32_t* ctx_out_len,
                        uint64_t* tail_len, void* stream);
/* kx_run_records_fd with the multi-byte split; the context carries from window to window (it starts empty). */
int kx_run_records_fd_rs(kx_program* p, int in_fd, int out_fd, const uint8_t* rs, uint32_t rs_len, int report_fd,
                         kx_records_stats* stats);

/* ---- record mode, framing apart from the program: strip the separator, append an output separator ---------------------------
 * kx_run_records_fd_opts is the four entry points above in one, plus:
 *   chomp    every record is run WITHOUT its separator (1 byte, or rs_len bytes in KX_RECORDS_RS mode).  A last record that is a
 *            tail has no valid separator and is run whole — under a quote or an escape byte it may end in a separator byte that
 *            is quoted or escaped: that byte is data and stays.  A record that is only its separator is the empty document: run,
 *            not skipped.  S of the report line counts inside the chomped record.
 *   ors      ors_len (0 to 8) bytes that follow the output of every accepted record (a tail and an empty output included); a
 *            rejected record writes nothing.  kx_records_stats::out_bytes counts them.
 * With a pipeline the separator is cut in front of stage 0 and ors added behind the last stage (kx_run_batch_framed).  With
 * chomp = 0 and ors_len = 0 the call is the entry point of its mode above.  `size` must be sizeof(kx_records_opts); the fields a
 * mode does not use are ignored, except that quote / escape are "-1: none" in KX_RECORDS_ESCAPED.  KX_E_ARG: a wrong size or mode,
 * what the mode's own entry point refuses, ors_len > 8, a non-zero reserved word. */
enum { KX_RECORDS_BYTE = 0, KX_RECORDS_QUOTED = 1, KX_RECORDS_ESCAPED = 2, KX_RECORDS_RS = 3 };
typedef struct kx_records_opts {
  uint32_t size;       /* sizeof(kx_records_opts) */
  uint32_t mode;       /* KX_RECORDS_* */
  uint8_t sep;         /* BYTE, QUOTED, ESCAPED */
  uint8_t pad[3];      /* must be 0 */
  int32_t quote;       /* QUOTED: a byte value; ESCAPED: a byte value or -1 */
  int32_t escape;      /* ESCAPED: a byte value */
  uint8_t rs[8];       /* RS */
  uint32_t rs_len;     /* RS: 1 to 8 */
  uint32_t chomp;      /* 0 / 1 */
  uint8_t ors[8];
  uint32_t ors_len;    /* 0 to 8 */
  uint32_t reserved[4];   /* must be 0 */
} kx_records_opts;
int kx_run_records_fd_opts(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, int report_fd, kx_records_stats* stats);

/* ---- field mode: the program runs on one field of every record, the rest of the record is copied ---------------------------------
 * kx_run_batch_fields is kx_run_batch where document i is FIELD `field` (counted from 1) of the record d_in[d_in_off[i], d_in_off[i+1]).
 * The record's BODY is its range without its last sep_len bytes (the record separator; with last_whole != 0 record n_docs - 1 has
 * none and is body to its end).  The body's fields lie between its live `fs` bytes: every one (quote = escape = -1); one at even
 * parity of the `quote` bytes before it IN THE RECORD (quote >= 0, escape = -1); one that is unescaped and at even parity of the
 * record's unescaped quotes (escape >= 0, quote a byte or -1) — the rules of the quoted and the escaped record split, from state 0
 * at the record's first byte.  A body with f live separators has f + 1 fields; the empty body has one empty field; nothing is
 * stripped from a field.  The program runs on the field as a whole input (every stage; its result is kx_run_device's for those
 * bytes alone), and
 *   accepted record i: its output d_out[d_out_off[i], d_out_off[i+1]) is body[0, field begin) + the program's output +
 *     body[field end, body end) + the record's own separator (keep_sep != 0, and the record has one) + suffix[0, suffix_len);
 *     d_docs[i] = {0, 0, 0}
 *   record i rejected by the program: its output range is empty; d_docs[i] = {fail_pos, 1, fail_stage}, fail_pos counted in the field
 *   record i with fewer than `field` fields: its output range is empty; d_docs[i] = {fields found, 2, 0}; the program is not run on
 *     it.  It counts as rejected (the return code, stats->docs_rejected).
 * Return codes, KX_E_CAPACITY with *out_len = the spliced bytes needed (d_out_off and d_docs are filled; d_out = NULL, cap = 0 is
 * the size query), the routed and replayed documents and everything else are kx_run_batch's.  KX_E_ARG besides: decreasing offsets
 * or a range shorter than sep_len other than a whole last one (found on the device before any kernel reads a record); a wrong
 * `size`, field = 0, fs equal to quote or escape, quote = escape, sep_len or suffix_len > 8, a non-zero reserved word (found before
 * any device work).  Per call the library holds 48 bytes of workspace per record, the fields' bytes and the program's output. */
typedef struct kx_batch_fields {
  uint32_t size;         /* sizeof(kx_batch_fields) */
  uint32_t field;        /* K: 1 to 2^32 - 1 */
  uint8_t fs;            /* the field separator */
  uint8_t pad[3];        /* must be 0 */
  int32_t quote;         /* a byte value, or -1: none */
  int32_t escape;        /* a byte value, or -1: none */
  uint32_t sep_len;      /* 0 to 8: the last sep_len bytes of every range are the record's separator */
  uint32_t last_whole;   /* != 0: the last record has no separator */
  uint32_t keep_sep;     /* != 0: a record's separator follows its output */
  uint32_t suffix_len;   /* 0 to 8 */
  uint8_t suffix[8];
  uint32_t reserved[4];  /* must be 0 */
} kx_batch_fields;
int kx_run_batch_fields(kx_program* prog, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_fields* fields,
                        void* d_out, size_t cap, uint64_t* d_out_off, kx_batch_doc* d_docs, size_t* out_len, kx_batch_stats* stats,
                        void* stream);
/* HIP-event times of field mode's own kernels (locate; gather; the two scans, the second with the kernel that measures the
   records' outputs; splice), summed over the program's kx_run_batch_fields calls so far; with kx_config::collect_timing, else 0. */
typedef struct kx_fields_kernel_stats {
  float locate_ms, gather_ms, scan_ms, splice_ms;
  uint64_t calls;
} kx_fields_kernel_stats;
int kx_fields_stats(const kx_program* prog, kx_fields_kernel_stats* out);

/* kx_run_records_fd_opts in field mode (`BIN --records … --field=K --fs=F`): every record the split of `o` delivers goes through
 * kx_run_batch_fields with field K = `field` (1 to 2^32 - 1) and the field separator `fs` — the quote and the escape byte of the
 * split decide which fs bytes are live, the separator (1 byte, or rs_len) is never part of the body, whether or not o->chomp is
 * set, the stream's tail has none.  An accepted record writes body[0, field) + the program's output + body[field end, end), then its
 * own separator unless o->chomp (a tail has none), then o->ors.  A record the program rejects writes nothing and reports
 * "Match error at input symbol S in record R!" with S counted inside the field; a record with fewer than K fields writes nothing,
 * reports "Record R has no field K!" and counts in records_rejected.  KX_E_ARG besides kx_run_records_fd_opts's: field = 0, fs equal
 * to the one-byte record separator (sep, or rs with rs_len = 1), to the quote or to the escape byte of the mode (a byte of a multi-byte
 * rs may equal fs). */
int kx_run_records_fd_fields(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, uint32_t field, uint8_t fs, int report_fd,
                             kx_records_stats* stats);

/* ---- field mode with a list of fields: the program runs on every selected field of a record, the rest is copied ------------------
 * kx_run_batch_field_list is kx_run_batch_fields in everything not said here: the records, their bodies, the live `fs` bytes, the
 * field numbering, sep_len, last_whole, keep_sep and the suffix are the same.  The selected set S is the union of `ranges` (the
 * NORMAL FORM of a `--field=LIST`: sorted, disjoint, not adjacent; hi = 0 means lo and every field behind it, and only the last
 * range may be open).  `need` is the largest number S names explicitly: the largest closed bound, or the open range's lo.
 *   record i with at least `need` fields: every field whose number is in S is run as a whole input of its own (every stage; its
 *     result is kx_run_device's for those bytes alone; each field of a range is a document of its own, the fs bytes between them
 *     are copied bytes).  If every one is accepted, the record's output is its body with every selected field replaced by the
 *     program's output for it + its own separator (keep_sep != 0, and the record has one) + suffix; d_docs[i] = {0, 0, 0}.
 *     Otherwise its output range is empty and d_docs[i] = {fail_pos, 1, fail_stage} of the LOWEST rejected field, fail_pos counted
 *     inside that field.
 *   record i with fewer than `need` fields: its output range is empty; d_docs[i] = {fields found, 2, 0}; the program runs on none
 *     of its fields.  It counts as rejected.
 * d_fail_field (a device array of n_docs uint32_t, or NULL): the field number K of the record's report line — the lowest rejected
 * field, or the smallest member of S above the fields the record has — and 0 for an accepted record.  n_docs, d_docs, d_out_off,
 * stats->docs and stats->docs_rejected count RECORDS; stats->docs_routed and docs_replayed are the inner kx_run_batch's and count
 * field runs.  KX_E_ARG besides kx_run_batch_fields's (a wrong `size`, the quote, escape, fs, sep_len, suffix_len and reserved-word
 * rules: before any device work; decreasing offsets and short ranges: on the device before any kernel reads a record): a list that
 * is not in normal form or has no or more than 8 ranges (before any device work), and a call whose records select more than
 * 2^32 - 2 fields in total (the inner batch's limit).  Per call the library holds 32 bytes of workspace per record, 64 per selected
 * field, the selected fields' bytes and the program's output. */
typedef struct kx_field_range { uint32_t lo, hi; } kx_field_range;   /* hi = 0: open (lo and everything behind it) */
typedef struct kx_batch_field_list {
  uint32_t size;         /* sizeof(kx_batch_field_list) */
  uint32_t n_ranges;     /* 1 to 8 */
  kx_field_range ranges[8];   /* the normal form: lo >= 1; hi == 0 or hi >= lo; ranges[j+1].lo > ranges[j].hi + 1; only the last may be open */
  uint8_t fs;            /* the field separator */
  uint8_t pad[3];        /* must be 0 */
  int32_t quote;         /* a byte value, or -1: none */
  int32_t escape;        /* a byte value, or -1: none */
  uint32_t sep_len;      /* 0 to 8: the last sep_len bytes of every range are the record's separator */
  uint32_t last_whole;   /* != 0: the last record has no separator */
  uint32_t keep_sep;     /* != 0: a record's separator follows its output */
  uint32_t suffix_len;   /* 0 to 8 */
  uint8_t suffix[8];
  uint32_t reserved[4];  /* must be 0 */
} kx_batch_field_list;
int kx_run_batch_field_list(kx_program* prog, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_field_list* list,
                            void* d_out, size_t cap, uint64_t* d_out_off, kx_batch_doc* d_docs, uint32_t* d_fail_field, size_t* out_len,
                            kx_batch_stats* stats, void* stream);

/* kx_run_records_fd_fields with a list (`BIN --records … --field=LIST [--fs=F]`): every record goes through kx_run_batch_field_list
 * with ranges[0, n_ranges) (the normal form, as above).  A record with too few fields reports "Record R has no field K!", a record
 * with a rejected field reports ONCE, "Match error at input symbol S in field K of record R!" with K the lowest rejected field and
 * S counted inside it; both write nothing and count in records_rejected.  KX_E_ARG: kx_run_records_fd_fields's, and a list that is
 * not in normal form. */
int kx_run_records_fd_field_list(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, const kx_field_range* ranges,
                                 uint32_t n_ranges, uint8_t fs, int report_fd, kx_records_stats* stats);

/* ---- field mode on unquoted values: the program runs on the VALUE of every selected field, the field is re-spelled -----------------
 * kx_run_batch_field_values is kx_run_batch_field_list in everything not said here: the records, the live `fs` bytes, the list, `need`,
 * "all selected fields accepted or nothing", return codes, KX_E_CAPACITY and the size query, d_docs, d_fail_field and the statistics.
 *   The program runs on the VALUE of a selected field (host.unquote_field_model): the field's bytes without the quote bytes that
 *     open and close quoted stretches and without the escape bytes; a quote that opens right behind one that closed (the "" of a
 *     quoted field) is one quote byte of the value; the byte behind an unescaped escape byte is data, a last escape byte alone is
 *     dropped.  The rule is total: a quote in the middle of a field toggles the state, an unclosed one is simply dropped.  fail_pos
 *     counts inside the value.
 *   An accepted record's selected fields are replaced by the SPELLING of the program's outputs (host.requote_field_model).  `special`
 *     are the bytes that must not appear bare (the records driver passes the record separator); was_quoted: the list has a quote byte
 *     and the raw field begins with it.  Quote, no escape: the output is wrapped iff was_quoted or it holds fs, the quote or a special
 *     byte — the quote byte, the output with every quote byte doubled, the quote byte; else it goes out as it is.  Escape: every
 *     escape byte gets an escape byte in front of it; with a quote every quote byte too, and the result is wrapped in quote bytes iff
 *     was_quoted or the output holds fs or a special byte; without a quote every fs and every special byte gets one as well.  An
 *     accepted empty output of a quoted field is two quote bytes.
 * KX_E_ARG besides kx_run_batch_field_list's, before any device work: a null codec or a wrong `size`, n_special > 8, a non-zero
 * reserved word, a special byte equal to the quote or the escape byte, a list with quote = escape = -1.  Per call the library holds,
 * beside kx_run_batch_field_list's workspace, 17 bytes per selected field, the values' bytes and the spellings' bytes. */
typedef struct kx_field_codec { uint32_t size; uint32_t n_special; uint8_t special[8]; uint32_t reserved[4]; } kx_field_codec;
int kx_run_batch_field_values(kx_program* prog, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_field_list* list,
                              const kx_field_codec* codec, void* d_out, size_t cap, uint64_t* d_out_off, kx_batch_doc* d_docs,
                              uint32_t* d_fail_field, size_t* out_len, kx_batch_stats* stats, void* stream);

/* kx_run_records_fd_field_list on values (`BIN --records … --quote|--escape --field=K|LIST [--fs=F] --unquote`): every record goes
 * through kx_run_batch_field_values with special = {o->sep}.  A rejected field always reports "Match error at input symbol S in field
 * K of record R!", S counted inside the value.  KX_E_ARG: kx_run_records_fd_field_list's, and a mode other than KX_RECORDS_QUOTED and
 * KX_RECORDS_ESCAPED. */
int kx_run_records_fd_field_values(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, const kx_field_range* ranges,
                                   uint32_t n_ranges, uint8_t fs, int report_fd, kx_records_stats* stats);

/* ---- field mode on words: the fields are the runs of bytes between blanks, as awk's default splitting has them ----------------------
 * kx_run_batch_field_words is kx_run_batch_field_list — with a codec, kx_run_batch_field_values — in everything not said here; the
 * normative text is host.blank_field_list_records_model.  A BLANK is the byte 0x20 or 0x09.  A blank is LIVE under the rule that
 * makes an `fs` byte live there: every one (quote = escape = -1); one at even parity of the `quote` bytes before it in the record;
 * one that is unescaped and at even parity of the record's unescaped quotes.  The body's fields are its WORDS, the maximal runs of
 * body bytes that are not live blanks, numbered from 1: a field is never empty, quotes and escapes stay in the word, and a body
 * that is empty or all live blanks has 0 fields — d_docs[i] = {fields found, 2, 0} may hold 0, and d_fail_field[i] is then the
 * list's first member.  An accepted record's output is its body with every selected word replaced (by the program's output, or
 * with a codec by its spelling); every other byte is copied as it is, every blank included — leading, trailing or repeated.
 *   list->fs must be 0 (the struct keeps its layout; the field is not used).
 *   codec may be NULL: the program runs on the raw words.  With a codec the value rule is unchanged and the spelling is
 *     requote_field_model's with fs = the space and `special` = the codec's bytes plus the tab, which the library appends: with a
 *     quote, an output that holds a blank is wrapped in quotes; with an escape and no quote, every blank of it gets an escape byte.
 * KX_E_ARG besides kx_run_batch_field_list's and, with a codec, kx_run_batch_field_values's, all before any device work: fs != 0;
 * a quote, an escape or a special byte that is a blank; n_special > 7. */
int kx_run_batch_field_words(kx_program* prog, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_field_list* list,
                             const kx_field_codec* codec, void* d_out, size_t cap, uint64_t* d_out_off, kx_batch_doc* d_docs,
                             uint32_t* d_fail_field, size_t* out_len, kx_batch_stats* stats, void* stream);

/* kx_run_records_fd_field_list on words (`BIN --records … --field=K|LIST --blanks [--unquote]`): every record goes through
 * kx_run_batch_field_words with ranges[0, n_ranges) — without a codec, or with unquote != 0 with special = {o->sep}.  The report lines
 * are kx_run_records_fd_field_list's; a record without any word reports "Record R has no field K!" with K the list's first member.
 * KX_E_ARG: kx_run_records_fd_opts's, a list that is not in normal form, a one-byte record separator (sep, or rs with rs_len = 1),
 * a quote or an escape byte of the mode that is a blank (a byte of a multi-byte rs may be one), and unquote != 0 in a mode other
 * than KX_RECORDS_QUOTED and KX_RECORDS_ESCAPED. */
int kx_run_records_fd_field_words(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, const kx_field_range* ranges,
                                  uint32_t n_ranges, int unquote, int report_fd, kx_records_stats* stats);

/* ---- field mode, projected: an accepted record writes the outputs of its selected fields alone, in the order the list was written ---
 * kx_run_batch_field_project is kx_run_batch_field_list — with KX_PROJECT_WORDS kx_run_batch_field_words, with a codec
 * kx_run_batch_field_values as well — in everything not said here; the normative text is host.project_records_model.  `proj->items`
 * is the list AS WRITTEN: 1 to 16 items lo-hi (hi = 0: lo and every field behind it) in any order, which may overlap and repeat.
 * The selected set S is their union, and `list` carries it and the framing: list->ranges MUST be the normal form of the items'
 * union (kx_field_list.h has the normaliser).  `need`, the records with too few fields, "every member of S runs once, all accepted
 * or nothing is written", d_docs, d_fail_field (the lowest rejected field NUMBER, whatever the written order), the return codes,
 * KX_E_CAPACITY and the size query are that call's.
 *   accepted record i: its output is, for each item in written order, the outputs of the item's fields in ascending field number
 *     (an open item: up to the record's last field; with a codec: their spellings), every two consecutive ones joined by
 *     ofs[0, ofs_len) + its own separator (keep_sep != 0, and the record has one) + suffix.  No byte of the body outside the
 *     selected fields is written; a field that two items name is written twice from its one run.
 *   With a codec the spelling protects the OUTPUT delimiter: requote_field_model's `fs` is ofs[0]; the special bytes are the
 *     codec's (plus the tab with KX_PROJECT_WORDS).
 * The statistics speak of the projected bytes.  KX_E_ARG besides that call's, before any device work: a null proj or a wrong
 * `size`, 0 or more than 16 items, an item with lo = 0 or 0 < hi < lo, ofs_len > 8, unknown flag bits, a non-zero reserved word,
 * ranges that are not the items' union; with a codec ofs_len != 1 or an OFS byte equal to the quote, the escape or a special byte.
 * Beside that call's workspace the library holds 256 bytes for the items' table. */
#define KX_PROJECT_WORDS 1u     /* the fields are the body's words (kx_run_batch_field_words; list->fs must be 0) */
#define KX_PROJECT_UNQUOTE 2u   /* kx_run_records_fd_field_project only: the program runs on the fields' values */
typedef struct kx_field_project {
  uint32_t size;         /* sizeof(kx_field_project) */
  uint32_t n_items;      /* 1 to 16 */
  kx_field_range items[16];   /* as written: lo >= 1; hi == 0 (open) or hi >= lo */
  uint32_t ofs_len;      /* 0 to 8 */
  uint8_t ofs[8];        /* the output field separator */
  uint32_t flags;        /* KX_PROJECT_WORDS */
  uint32_t reserved[4];  /* must be 0 */
} kx_field_project;
int kx_run_batch_field_project(kx_program* prog, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_field_list* list,
                               const kx_field_codec* codec /* or NULL */, const kx_field_project* proj, void* d_out, size_t cap,
                               uint64_t* d_out_off, kx_batch_doc* d_docs, uint32_t* d_fail_field, size_t* out_len, kx_batch_stats* stats,
                               void* stream);

/* kx_run_records_fd_field_list, projected (`BIN --records … --field=K|LIST [--fs=F | --blanks] [--unquote] --only [--ofs=STR]`): every
 * record goes through kx_run_batch_field_project with items[0, n_items) as written, the normal form of their union for the list
 * and ofs[0, ofs_len).  flags: KX_PROJECT_WORDS (the fields are words; `fs` is not used) and KX_PROJECT_UNQUOTE (with a codec whose
 * special byte is o->sep).  The report lines are kx_run_records_fd_field_list's.  KX_E_ARG: the rules of the entry point the flags
 * name (kx_run_records_fd_field_list, _field_values, _field_words), invalid items or more than 16, a union of more than 8 ranges,
 * ofs_len > 8, unknown flag bits, and with KX_PROJECT_UNQUOTE an OFS that is not one byte or equals the quote, the escape or the
 * record separator. */
int kx_run_records_fd_field_project(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, const kx_field_range* items,
                                    uint32_t n_items, uint8_t fs, const uint8_t* ofs, uint32_t ofs_len, uint32_t flags, int report_fd,
                                    kx_records_stats* stats);

/* ---- header rows, and fields selected by column name (`BIN --records --header[=N] [--field=LIST with names] …`) -------------------
 * The first `header` records of the stream are HEADER records: the program never runs on them, R of the report lines and
 * kx_records_stats::records count them.  Without KX_TABLE_ONLY each is written as its body, its own separator unless o->chomp (a
 * tail has none), then o->ors; nothing is looked for in it.  With KX_TABLE_ONLY it is projected as an accepted data record whose
 * program is the identity (kx_run_batch_field_header); one with fewer than `need` cells is reported "Record R has no field K!",
 * writes nothing and counts as rejected.
 *   An item with lo == 0 is a NAME, names[hi][0, name_len[hi]).  Names are resolved once, when header record `header` is in hand:
 * its body's cells are cut by the live `fs` bytes of o's mode (KX_TABLE_WORDS: into words); a cell's name is its bytes, and with a
 * quote or an escape byte its value (host.unquote_field_model), with or without KX_TABLE_UNQUOTE; if that record is the stream's
 * first and begins with EF BB BF, the names are cut behind those bytes.  A name selects the lowest-numbered cell that has it.  From
 * then on the run is that of the same items as numbers; a list with a name always reports "… in field K of record R!".  With
 * KX_TABLE_ONLY and names, the header records in front of record `header` are held until it has come: a stream that ends before
 * it writes none of them.  A name no cell has, or a resolved union of more than 8 ranges: KX_E_HEADER, no byte of record `header`
 * or of anything behind it is written, and kx_last_error names the entry point and the name.  A stream that ends before record
 * `header` resolves nothing and returns 0.
 *   With header == 0 (names are then refused) the call is exactly the entry point its flags name: no items kx_run_records_fd_opts;
 * KX_TABLE_SINGLE kx_run_records_fd_fields; KX_TABLE_ONLY kx_run_records_fd_field_project with the items as written; else
 * KX_TABLE_WORDS kx_run_records_fd_field_words, KX_TABLE_UNQUOTE kx_run_records_fd_field_values, no flag
 * kx_run_records_fd_field_list, each with the normal form of the items' union.
 * KX_E_ARG before any device work: those entry points' own refusals; a wrong `size`; non-zero pad or reserved words; unknown flag
 * bits; flags without items; more than 16 items or names; an item with lo >= 1 and 0 < hi < lo; a name index >= n_names; a name of
 * 0 or more than 255 bytes; a null name pointer; names with header == 0; KX_TABLE_SINGLE with another flag or with anything but
 * one closed number item; without names, a union of more than 8 ranges. */
#define KX_E_HEADER (-6)        /* a name of the field list is no cell of the header record, or the resolved list has too many ranges */
#define KX_TABLE_WORDS 1u       /* the fields are the words between blanks (`fs` is not used) */
#define KX_TABLE_UNQUOTE 2u     /* the program runs on the fields' values */
#define KX_TABLE_ONLY 4u        /* only the selected fields are written, in the items' order, joined by ofs */
#define KX_TABLE_SINGLE 8u      /* one item K-K that reports as kx_run_records_fd_fields ("… in record R!") */
typedef struct kx_records_table {
  uint32_t size;              /* sizeof(kx_records_table) */
  uint32_t header;            /* N: the first N records are header records (0: none) */
  uint32_t flags;             /* KX_TABLE_* */
  uint32_t n_items;           /* 0: no field mode */
  kx_field_range items[16];   /* as written.  lo >= 1: numbers, as in kx_field_project; lo == 0: the name names[hi] */
  uint32_t n_names;
  const uint8_t* names[16];
  uint32_t name_len[16];      /* 1 to 255 */
  uint8_t fs;                 /* the field separator (not with KX_TABLE_WORDS) */
  uint8_t pad[3];             /* must be 0 */
  uint32_t ofs_len;           /* KX_TABLE_ONLY: 0 to 8 */
  uint8_t ofs[8];
  uint32_t reserved[4];       /* must be 0 */
} kx_records_table;
int kx_run_records_fd_table(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, const kx_records_table* t, int report_fd,
                            kx_records_stats* stats);

/* kx_run_batch_field_project in every word of its contract, with the identity in the program's place for every record of the call:
 * the selected fields themselves (with a codec: the spellings of their values) are what is projected, no record is ever rejected
 * by the program (status 2, too few fields, remains), and no document is routed or replayed.  It is the route a header record takes
 * under KX_TABLE_ONLY. */
int kx_run_batch_field_header(kx_program* prog, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_field_list* list,
                              const kx_field_codec* codec /* or NULL */, const kx_field_project* proj, void* d_out, size_t cap,
                              uint64_t* d_out_off, kx_batch_doc* d_docs, uint32_t* d_fail_field, size_t* out_len, kx_batch_stats* stats,
                              void* stream);

/* ---- field mode by key: the fields are key=value pairs, and the program runs on the values of the listed keys ----------------------
 * (`BIN --records … --field=LIST --keys[=C]`; the normative text is host.keyed_records_model.)  kx_run_batch_field_keys is
 * kx_run_batch_field_list — with KX_KEYS_WORDS kx_run_batch_field_words, with a codec kx_run_batch_field_values, with `proj`
 * kx_run_batch_field_project — in everything not said here: the records, their bodies, how a body is cut into fields (the live
 * `fs` bytes; with KX_KEYS_WORDS the words between live blanks), sep_len, last_whole, keep_sep and the suffix, the codec's value
 * and spelling rules, return codes, KX_E_CAPACITY and the size query, and the statistics.  `list` carries that framing; its
 * n_ranges MUST be 0 (with KX_KEYS_WORDS its fs too).
 *   Inside a field the KEY is the bytes before the field's first live `kv` byte — live under the rule that makes an fs byte live,
 * with the record's running state — and the VALUE everything behind that byte up to the field's end; it may be empty.  A field
 * without a live kv byte has no key; an empty key matches nothing; keys are compared as raw bytes, quotes and escapes included.
 * Per record each name selects the FIRST field that has it for a key; later fields with that key are bytes like any other.
 *   The selected values are the record's documents, in address order: each is run as a whole input of its own (with a codec its
 * value, host.unquote_field_model; fail_pos counts inside it).
 *   A record that lacks a name whose bit is not set in optional_mask: its output range is empty, d_docs[i] = {the 16-bit mask of
 *     the names it has, 2, 0}, d_fail_field[i] = 1 + the index of the first such name; the program runs on none of its values.
 *   A record with a rejected value: its output range is empty, d_docs[i] = {fail_pos, 1, fail_stage} of the rejected value at the
 *     lowest address, d_fail_field[i] = 1 + the index of its name.
 *   Any other record is accepted, d_docs[i] = {0, 0, 0}, d_fail_field[i] = 0: its output is its body with each selected value
 *     replaced (key and kv byte are copied) + its own separator (keep_sep) + suffix; a record that holds none of the names — all
 *     of them optional — is written unchanged.  With `proj`: for each item in written order — proj->items[t] = {0, name index} —
 *     the output of that name's value, joined by ofs; an optional name the record lacks writes nothing and no ofs, and a record
 *     without any output writes its separator and the suffix alone.
 * `names` are the DISTINCT names in the order the list was written, so that "the first name it lacks" is the lowest index; with
 * `proj` every name index an item holds is below n_names.  KX_E_ARG besides those calls', before any device work: a null `keys` or
 * a wrong `size`; n_names = 0 or > 16; a null name, one of 0 or more than 255 bytes, two equal names; optional_mask bits at or
 * above n_names; unknown flag bits; a non-zero reserved word; list->n_ranges != 0; kv equal to fs (KX_KEYS_WORDS: a blank), the
 * quote or the escape byte; a name that holds kv or fs (KX_KEYS_WORDS: a blank); with `proj` a wrong size, 0 or more than 16
 * items, an item that is no {0, index < n_names}, ofs_len > 8, and with a codec too an ofs that is not one byte or equals the
 * quote, the escape or a special byte.  Beside kx_run_batch_field_list's workspace the library holds 4 144 bytes for the names'
 * table, a byte per document and with `proj` 16 bytes per record. */
#define KX_KEYS_WORDS 1u        /* the fields are the body's words (list->fs must be 0) */
#define KX_KEYS_UNQUOTE 2u      /* kx_run_records_fd_field_keys only: the program runs on the values' values (a codec with o->sep) */
#define KX_KEYS_ONLY 4u         /* kx_run_records_fd_field_keys only: items and ofs are a projection */
typedef struct kx_field_keys {
  uint32_t size;              /* sizeof(kx_field_keys) */
  uint32_t n_names;           /* 1 to 16 */
  const uint8_t* names[16];   /* distinct, in written order */
  uint32_t name_len[16];      /* 1 to 255 */
  uint32_t optional_mask;     /* bit t: a record may lack names[t] */
  uint8_t kv;                 /* the key separator C */
  uint8_t pad[3];             /* must be 0 */
  uint32_t flags;             /* KX_KEYS_WORDS */
  uint32_t reserved[4];       /* must be 0 */
} kx_field_keys;
int kx_run_batch_field_keys(kx_program* prog, const void* d_in, const uint64_t* d_in_off, uint64_t n_docs, const kx_batch_field_list* list,
                            const kx_field_keys* keys, const kx_field_codec* codec /* or NULL */, const kx_field_project* proj /* or NULL */,
                            void* d_out, size_t cap, uint64_t* d_out_off, kx_batch_doc* d_docs, uint32_t* d_fail_field, size_t* out_len,
                            kx_batch_stats* stats, void* stream);

/* kx_run_records_fd_field_list by key (`BIN --records … --field=LIST --keys[=C] [--fs=F | --blanks] [--unquote] [--only
 * [--ofs=STR]]`): every record goes through kx_run_batch_field_keys.  keys->flags: KX_KEYS_WORDS (`fs` is not used),
 * KX_KEYS_UNQUOTE (a codec whose special byte is o->sep) and KX_KEYS_ONLY (a projection of items[0, n_items), each an index into
 * keys->names, joined by ofs[0, ofs_len); without it items may be NULL).  A record that lacks a required name reports "Record R
 * has no field NAME!", NAME the first such name; a record with a rejected value reports once, "Match error at input symbol S in
 * field NAME of record R!"; both write nothing and count in records_rejected.  NAME is printed with its bytes outside 0x20 to
 * 0x7E as \xHH.  KX_E_ARG: kx_run_records_fd_field_list's (with KX_KEYS_WORDS _field_words's, with KX_KEYS_UNQUOTE
 * _field_values's, with KX_KEYS_ONLY _field_project's for the ofs), kx_run_batch_field_keys's for `keys`, and a kv or a name
 * byte equal to the one-byte record separator. */
int kx_run_records_fd_field_keys(kx_program* p, int in_fd, int out_fd, const kx_records_opts* o, const kx_field_keys* keys, uint8_t fs,
                                 const uint32_t* items, uint32_t n_items, const uint8_t* ofs, uint32_t ofs_len, int report_fd,
                                 kx_records_stats* stats);

/* ---- sharded execution: one contiguous shard of the input per GPU -------------
 * Per stage and per rank:
 *   kx_shard_begin → kx_shard_forward → [exchange kx_fwd_summary] → kx_shard_fix_head
 *   → kx_shard_backward → [exchange kx_bwd_summary, last rank first] → kx_shard_resolve
 *   → [exchange out_len] → kx_shard_emit → kx_shard_end
 * The only cross-shard data are the two fixed-size summaries below (the chunk-boundary
 * hand-off); the data path needs no collective. */
#define KX_MAX_LEAVES 256
typedef struct kx_fwd_summary {
  uint32_t synced;      /* 1: end_state does not depend on the incoming state                  */
  uint32_t end_state;   /* state entering the byte after this shard (valid if synced or fixed) */
  uint64_t head_len;    /* leading bytes that still need the incoming state (0 on first shard)  */
  uint64_t fail_pos;    /* UINT64_MAX = no failure seen so far                                 */
} kx_fwd_summary;
typedef struct kx_bwd_summary {
  uint32_t constant;                     /* 1: start leaf is the same for every end leaf */
  uint32_t nleaves;                      /* leaves of the state at the shard end         */
  uint8_t start_leaf[KX_MAX_LEAVES];     /* start leaf of the shard, per end leaf        */
} kx_bwd_summary;

int kx_shard_begin(kx_program* prog, uint32_t stage, const void* d_in, size_t n, int is_first, int is_last,
                   void* stream, kx_shard** shard);
int kx_shard_forward(kx_shard* s, kx_fwd_summary* out);
int kx_shard_fix_head(kx_shard* s, uint32_t incoming_state, kx_fwd_summary* out);
int kx_shard_backward(kx_shard* s, kx_bwd_summary* out);
int kx_shard_resolve(kx_shard* s, uint32_t end_leaf, uint64_t* out_len);
/* Writes the shard's out_len bytes (kx_shard_resolve's) to d_out and nothing outside d_out[0, out_len), whatever `cap` says.  d_out is
 * 16-byte aligned: KX_E_ARG otherwise; cap < out_len is KX_E_CAPACITY; d_out is untouched on both.  The shard's input (16-byte aligned,
 * kx_shard_begin) is never written, and no byte outside its [0, n) influences the result. */
int kx_shard_emit(kx_shard* s, void* d_out, size_t cap);
void kx_shard_stats(kx_shard* s, kx_stats* stats);
void kx_shard_end(kx_shard* s);

/* ---- the multi-GPU driver: the protocol above, run by the library itself ---------------------------------------
 * One rank per GPU (a process, or a thread of one process); rank r holds shard r of the input on its own current device.
 * kx_run_sharded runs every pipeline stage over the rank's shard and takes part in the boundary hand-off — four
 * all-gathers of fixed-size records per stage (40, 40, 272 and 16 bytes per rank; one more of 16 bytes behind the last stage's emit), nothing else crosses ranks — through
 * the all-gather it is given:
 *   kx_comm_*   RCCL: `ncclAllGather` on the communicator's own device buffers and stream (xGMI between the GPUs of a node;
 *               librccl is dlopen'ed).  Rank 0 makes the 128-byte id (kx_comm_unique_id) and the launcher hands it to every
 *               rank (ncclGetUniqueId / ncclCommInitRank's contract); every rank then calls kx_comm_init on its device.
 *   kx_group_*  the threads of one process (the produced binary's `--gpus N`): exchange through host memory.
 * With world = 1 no exchange takes place (ag may be NULL).  Returns as kx_run_device: 0, 1 (match error: res->stats.fail_pos
 * is the GLOBAL position, the same on every rank), or < 0 (KX_E_CAPACITY: res->out_len = bytes this rank needs).
 * The rank's output slice [out_offset, out_offset + out_len) of the total_out output bytes stays on its device. */
typedef int (*kx_allgather_fn)(void* ctx, const void* send, void* recv, size_t bytes);   /* recv holds world * bytes; 0 = ok */
typedef struct kx_sharded_result {
  uint64_t out_len, out_offset, total_out;
  float boundary_ms;   /* wall time this rank spent inside the all-gathers (waiting for the slowest rank included) */
  kx_stats stats;      /* kernel times summed over the stages; fail_pos / fail_stage on a match error */
} kx_sharded_result;
/* (collective return code: every record of the exchanges carries the sender's status and one more status word follows the last
 *  stage's emit, so a local failure — out of memory,
 *  a HIP error — ends the call on EVERY rank instead of leaving the others inside an all-gather) */
int kx_run_sharded(kx_program* prog, int rank, int world, kx_allgather_fn ag, void* ag_ctx, const void* d_in, size_t n,
                   void* d_out, size_t cap, kx_sharded_result* res, void* stream);

/* The produced binary's `--gpus N`: stdin must be a regular file; it is cut into N contiguous shards (4 KiB multiples), one
 * thread and one program instance per GPU, hand-off through host memory (kx_group_*); the output is written at each rank's
 * offset (regular file) or in rank order (pipe).  Same return codes and match-error position as kx_run_fd.
 * Limits: every rank holds its WHOLE shard and its output in device memory (no windows, unlike kx_run_fd): an input beyond
 * about N x 100 GB fails with "cannot place the shard on the device".  stats: kernel times of the slowest rank, counts summed.
 * The return code is collective (kx_run_sharded): a rank that fails locally says so in the next exchange and every rank
 * returns — its own code and message, or KX_E_IO naming the failing rank. */
int kx_run_fd_sharded(const void* blob, size_t blob_len, int ngpus, int in_fd, int out_fd, kx_stats* stats);
int kx_run_fd_sharded_cfg(const void* blob, size_t blob_len, const kx_config* cfg, int ngpus, int in_fd, int out_fd, kx_stats* stats);

typedef struct kx_comm kx_comm;
int kx_comm_unique_id(void* id128);
int kx_comm_init(kx_comm** comm, int rank, int world, const void* id128);
void kx_comm_free(kx_comm* comm);
int kx_comm_allgather(void* comm, const void* send, void* recv, size_t bytes);            /* a kx_allgather_fn */

typedef struct kx_group kx_group;
typedef struct kx_group_member kx_group_member;
kx_group* kx_group_create(int world);
void kx_group_free(kx_group* g);
kx_group_member* kx_group_join(kx_group* g, int rank);
void kx_group_leave(kx_group_member* m);
void kx_group_abort(kx_group* g);   /* a member that fails outside the protocol wakes the others: their all-gathers return an error */
int kx_group_allgather(void* member, const void* send, void* recv, size_t bytes);         /* a kx_allgather_fn */

#ifdef __cplusplus
}
#endif
#endif
