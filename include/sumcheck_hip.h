/* sumcheck_hip.h -- C ABI of libsumcheck_hip.so: the MI355X (gfx950) prover hot path of the
 * linear-time multilinear sumcheck, a drop-in for arkworks-rs/sumcheck's
 *   IPForMLSumcheck::{prover_init, prove_round}      (reference src/ml_sumcheck/protocol/prover.rs:49,74)
 *   DenseMultilinearExtension::fix_variables          (ark-poly; called at prover.rs:88)
 *   MLSumcheck::{prove, prove_as_subprotocol}         (reference src/ml_sumcheck/mod.rs:42,50)
 *   gkr_round_sumcheck::{initialize_phase_one, initialize_phase_two, GKRRoundSumcheck::prove}
 *                                                      (reference src/gkr_round_sumcheck/mod.rs:22,57,93)
 *
 * The reference has no FFI of its own (it is pure Rust with #![forbid(unsafe_code)], src/lib.rs:1);
 * these entry points are what a Rust `extern "C"` shim crate binds (INTEGRATION.md shows the stub).
 *
 * ELEMENT LAYOUT.  A field element is `uint64_t[4]`: the little-endian limbs of the MONTGOMERY form
 * (R = 2^256) of a BLS12-381 scalar, always < p -- bit-for-bit the in-memory layout of
 * ark_ff::Fp<MontBackend<FrConfig,4>,4>, so `evaluations.as_ptr() as *const u64` can be passed
 * straight in and outputs can be wrapped back into `Fp` without conversion.  A table of 2^nv
 * evaluations is 2^nv * 32 contiguous bytes, index bit k <-> variable k (ark-poly
 * DenseMultilinearExtension).
 *
 * OWNERSHIP.  sc_prover_init copies its inputs (as prover_init deep-copies, prover.rs:55-59) unless
 * SC_TABLES_BORROW is set; it never writes caller memory.  Device tables that are COPIED (init or reset) are read after a
 * device-wide synchronise, so work still in flight on the caller's streams that produces them is waited for.  BORROWED device
 * tables are read by kernels on the handle's stream: the caller must have synchronised their producer before the first round.  A handle owns its device memory until
 * sc_prover_free.  Outputs go to caller-owned host buffers unless the parameter says "device".
 *
 * THREADING.  One handle = one host thread at a time.  Distinct handles are independent and may be used from different threads
 * concurrently, on one GPU or several; the library serialises its own HIP calls per device (a pipelined round must never find
 * the launch that follows its wait kernel blocked behind another thread's call), so threads sharing a GPU take turns at the
 * granularity of one round.  Calls are synchronous (return after the result is on the host) unless named *_async / *_partial.
 *
 * ERRORS.  Nothing aborts across the ABI.  The four misuse panics of the reference map to status codes
 * (the shim turns them back into the same panic! messages); sc_last_error() gives detail.
 * There is NO CPU fallback: without a usable HIP device every compute entry point returns SC_ERR_HIP.  A call that fails on a HIP error
 * (SC_ERR_OOM: an allocation was refused; SC_ERR_HIP) takes that error out of the runtime's per-thread "last error" slot, so it does not
 * resurface in the next call; the handle it failed on is freed (init) or must be reset (a proof in progress).
 */
#ifndef SUMCHECK_HIP_H
#define SUMCHECK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_ABI_VERSION 5 /* 5: sc_set_policy, sc_get_policy, sc_plan_count, sc_plan_name, sc_plan_stats (additions only), and later, still within 5, sc_ml_prove_batch, sc_gkr_prove_batch, sc_poly_evaluate_batch, sc_gkr_subclaim_batch, the sc_batch_prover_* family and the sc_gkr_batch_prover_* family with sc_gkr_batch_prove_round, sc_gkr_layer_next_batch, and sc_gkr_two_point_init_batch with sc_gkr_two_point_next_batch, sc_gkr_layers_eval_batch, and sc_gkr_gates_init_batch with sc_gkr_gates_next_batch and sc_gkr_gates_layers_eval_batch (additions: a caller detects the symbol itself); 4: sc_comm_info, sc_comm_exchange_bench, sc_set_publish_timeout_ms, sc_prover_get_round_timing, sc_library_stats (additions only); 3: sc_prover_set_polling, sc_prover_set_resident, SC_NO_DEVICE_POLLING, sc_set_cache_limit, sc_comm_init_p2p, sc_gkr_prove_sharded (additions only) */
#define SC_API __attribute__((visibility("default")))

enum sc_status {
    SC_OK = 0,
    SC_ERR_CONSTANT_POLY = 1,       /* "Attempt to prove a constant."        prover.rs:50-52 */
    SC_ERR_FIRST_ROUND_HAS_MSG = 2, /* "first round should be prover first." prover.rs:79-81 */
    SC_ERR_MISSING_MSG = 3,         /* "verifier message is empty"           prover.rs:90-92 */
    SC_ERR_NOT_ACTIVE = 4,          /* "Prover is not active"                prover.rs:96-98 */
    SC_ERR_BAD_ARG = 5,             /* assert!/assert_eq! failures of data_structures.rs:78-84 and gkr mod.rs:28-29,61 */
    SC_ERR_HIP = 6,                 /* HIP runtime failure or no device */
    SC_ERR_OOM = 7,
    SC_ERR_REJECT = 8               /* verifier: "Prover message is not consistent with the claim." verifier.rs:107-113 */
};

enum sc_flags {
    SC_TABLES_ON_DEVICE = 1u << 0, /* `tables[]` are device pointers (HBM-resident), not host */
    SC_TABLES_BORROW = 1u << 1,    /* with ON_DEVICE: do not copy; tables are only read and must outlive the handle */
    SC_TABLES_STREAM = 1u << 2,    /* HOST tables too large to copy: see sc_prover_init_streamed (set by it; sc_prover_init accepts it too) */
    SC_NO_DEVICE_POLLING = 1u << 3 /* this handle never parks a kernel on the GPU that waits for the host (sc_prover_set_polling(p, 0) from the start) */
};

/* Flattened ListOfProductsOfPolynomials (reference src/ml_sumcheck/data_structures.rs:25-35):
 * products[k] = (coeffs[k], prod_indices[prod_offsets[k] .. prod_offsets[k+1]]) indexing `tables`. */
typedef struct sc_poly_desc {
    uint32_t num_vars;            /* num_variables */
    uint32_t max_multiplicands;   /* must equal max_k m_k (data_structures.rs:79) */
    uint32_t n_products;          /* K */
    const uint64_t *coeffs;       /* K x 4 limbs (host) */
    const uint32_t *prod_offsets; /* K+1 (host) */
    const uint32_t *prod_indices; /* sum m_k entries (host), each < n_tables */
    uint32_t n_tables;            /* U = flattened_ml_extensions.len() */
    const uint64_t *const *tables;/* U pointers, each 2^num_vars x 4 limbs */
    uint32_t flags;               /* sc_flags */
} sc_poly_desc;

typedef struct sc_prover sc_prover; /* ProverState (prover.rs:19-33) with tables resident in HBM */
typedef struct sc_rng sc_rng;       /* Blake2b512Rng (reference src/rng.rs:22-25) */

/* ---- library ------------------------------------------------------------------------------- */
SC_API int sc_abi_version(void);
SC_API const char *sc_last_error(void);     /* thread-local, valid until the next call on this thread */
SC_API int sc_device_count(void);           /* number of visible HIP devices (0 => every compute call fails) */
SC_API int sc_set_device(int ordinal);      /* device used by handles created afterwards on this thread */

/* ---- IPForMLSumcheck::prover_init / prove_round (prover.rs:49-153) ------------------------- */
SC_API int sc_prover_init(const sc_poly_desc *desc, sc_prover **out);
/* Out-of-core tables: the tables stay in HOST memory (pinned memory streams fastest; they are only read and must
 * stay valid until the second round has returned) and are never resident as a whole.  Rounds 1 and 2 pull them through a two-slot
 * staging ring, 2^chunk_log2 entries of every table at a time (0 = 2^22; clamped to [2^10, 2^num_vars]), the copy of one chunk
 * overlapping the kernels of the previous one; from round 2 on the bound tables -- half the input -- are resident and everything
 * proceeds as usual.  HBM footprint: 0.84 x the tables (bound-table buffers) + 2 x U x 2^chunk_log2 x 32 bytes, instead of 2.7 x.
 * The input crosses PCIe twice (rounds 1 and 2 both need it and the challenge between them comes from the verifier).
 * Any product shape: up to 12 products of at most 4 multiplicands walk a chunk in one launch (the merged big-round kernel); other
 * shapes bind the chunk table by table and sum product by product.  Below 2^11 entries per table the handle silently copies instead.
 * Every other call (sc_prove_round, sc_prove_round_partial / sc_ml_prove_sharded -- each rank of a multi-GPU proof may stream its own
 * shard --, sc_ml_prove_handle, sc_prover_state, sc_prover_reset with host tables or NULL) works on the handle unchanged. */
SC_API int sc_prover_init_streamed(const sc_poly_desc *desc, uint32_t chunk_log2, sc_prover **out);
/* r_or_null: NULL exactly on the first call, else the previous round's challenge (4 limbs).
 * out_evals: (max_multiplicands+1) x 4 limbs = [P(0), P(1), ..., P(deg)] (ProverMsg, prover.rs:13-17). */
SC_API int sc_prove_round(sc_prover *p, const uint64_t *r_or_null, uint64_t *out_evals);
/* (Late rounds -- at most 2048 pairs -- of this round-by-round protocol do not pay a launch sequence each: the first of them launches
 * one kernel for all remaining rounds, which stays on the GPU polling a host-mapped mailbox; every following sc_prove_round posts
 * its challenge and takes the next message.  The kernel's patience is short, `patience_polls` polls of ~2 us (default 256; 0 = never
 * use a resident kernel): a verifier that takes longer finds it gone -- it leaves after the last round it completed -- and the call
 * proceeds with ordinary launches.  Any other call on the handle makes it leave first.  Not used while sc_prover_set_timing is on,
 * on a caller's stream, with sc_prover_set_polling(p, 0) / sc_set_policy("pipeline", 0), or with sc_set_policy("resident", 0).) */
SC_API int sc_prover_set_resident(sc_prover *p, uint32_t patience_polls);
/* MLSumcheck::prove_as_subprotocol pushes the final challenge without binding it (mod.rs:65-67). */
SC_API int sc_prover_push_randomness(sc_prover *p, const uint64_t *r);
/* Copy ProverState back to the host.  randomness: up to num_vars x 4 limbs (may be NULL);
 * tables_out: U x 2^(num_vars - bound) x 4 limbs, bound = max(round-1, 0) (may be NULL);
 * *round, *n_randomness may be NULL. */
SC_API int sc_prover_state(sc_prover *p, uint64_t *randomness, uint32_t *n_randomness, uint64_t *tables_out, uint32_t *round);
SC_API void sc_prover_free(sc_prover *p);
/* Run the handle's kernels on a caller stream (a hipStream_t cast to void*; NULL is the legacy default stream,
 * which is what torch.cuda.current_stream().cuda_stream is unless a side stream is active), or -- use_own != 0 --
 * back on the handle's own non-blocking stream. */
SC_API int sc_prover_set_stream(sc_prover *p, void *hip_stream, int use_own);
/* DEVICE-SIDE WAITS AND FOREIGN HIP TRAFFIC -- the interference contract.  Inside sc_ml_prove* / sc_gkr_prove the latency-bound rounds
 * are launched BEFORE their challenge exists: a one-wavefront kernel (k_wait_challenge) or the persistent tail kernel (k_tail_rounds)
 * sits on the handle's stream and polls a host-mapped word until the calling thread has hashed the previous message.  While such a
 * kernel waits, the calling thread must be able to finish its HIP calls.  The library's own threads are serialised per device (see
 * THREADING); HIP calls made by OTHER code of the process on the same device (hipMalloc / hipFree / synchronous copies take
 * process-wide locks inside the runtime) can hold the calling thread up.  What then happens, in this order:
 *   - nothing, if the delay is shorter than the wait's bound (seconds; policy "wait_spins"): the proof is slower, never different;
 *   - the wait expires: messages computed on a stale challenge are never returned.  A handle whose inputs are intact (borrowed or
 *     streamed tables) proves again from round 0 with synchronous rounds inside the same call; a copying handle returns SC_ERR_HIP
 *     ("... the proof is void") and must be reset with its tables.
 * A host that runs its own HIP work on the device concurrently (a Rust application with its own streams, an ML framework) should
 * switch the device-side waits off for its handles: allow = 0 makes every round of this handle launch after its challenge is known
 * (about 0.3 ms more per 24-variable proof, no kernel ever waits for the host, nothing can expire).  sc_set_policy("pipeline", 0)
 * does the same for every handle of the process.  Returns SC_OK; the setting holds until changed. */
SC_API int sc_prover_set_polling(sc_prover *p, int allow);

/* Sharded use: this handle holds one contiguous high-bit shard of every table.
 * sc_prove_round_partial = prove_round on the shard, result left ON THE DEVICE as (deg+1) x 8 uint64
 * lanes, lane j of evaluation t = 32-bit limb j zero-extended -- summable across ranks with an integer
 * all-reduce (no modular all-reduce exists); asynchronous on the handle's stream.
 * sc_wide_reduce folds summed lanes (host) back to canonical Montgomery limbs. */
SC_API int sc_prove_round_partial(sc_prover *p, const uint64_t *r_or_null, uint64_t *d_wide_out);
SC_API int sc_wide_reduce(const uint64_t *wide, uint32_t n_elems, uint64_t *out);
/* Bind the last local variable: tables of 2 entries -> 1 entry each, written to d_out (U x 4 limbs,
 * device), asynchronous on the handle's stream.  After this the handle is exhausted. */
SC_API int sc_prover_bind_final(sc_prover *p, const uint64_t *r, uint64_t *d_out);

/* Multi-GPU proofs inside the library.  PROCESS MODEL: one sc_prover per GPU, each holding one contiguous
 * high-bit shard of every table (rank g: entries [g * 2^nv_local, (g+1) * 2^nv_local)), driven by one host thread per GPU --
 * either one process per GPU (torchrun, MPI) or one thread per GPU inside one process (sc_set_device is per thread; this is how
 * a Rust host would use it).  There is no single-handle "n_gpus" mode: every rank runs the same call and they meet in the
 * collectives.  A communicator is
 *   - an RCCL one: rank 0 creates the 128-byte unique id (sc_comm_unique_id) and ships it to the other ranks by any means;
 *     every rank then calls sc_comm_init on its own device.  RCCL is bound at run time (dlopen).  The per-round all-reduce
 *     (sum, uint64, (deg+1) x 8 lanes) and the tail's all-gather run on the handle's stream;
 *   - or a HOST transport (sc_comm_init_host): two caller functions that exchange small host buffers (MPI, gloo, shared
 *     memory between threads, ...).  allreduce sums `count` uint64 words in place over all ranks; allgather delivers every
 *     rank's `bytes` bytes in rank order into recv (nranks * bytes).  Both return 0 on success.
 * sc_ml_prove_sharded = MLSumcheck::prove_as_subprotocol (mod.rs:50-70) for the GLOBAL instance of nv_total variables: the
 * nv_total - log2(nranks) local rounds, then bind + all-gather + the last log2(nranks) rounds on the gathered tables.
 * p: this rank's shard, at round 0.  out_proof: nv_total x (deg+1) x 4, out_randomness: nv_total x 4 -- identical on every
 * rank.  rng_or_null: NULL = a fresh transcript.  nranks must be a power of two.  Every rank of a group uses the same kind of handle
 * (all resident or all streamed: the point where the sharding stops depends on it).
 * sc_ml_prove_sharded_rounds: only the first n_rounds local rounds (PolynomialInfo of the global instance is fed first). */
typedef struct sc_comm sc_comm;
typedef int (*sc_allreduce_u64_fn)(void *ctx, uint64_t *inout, size_t count);
typedef int (*sc_allgather_fn)(void *ctx, const void *send, void *recv, size_t bytes);
SC_API int sc_comm_unique_id(uint8_t *out128);
SC_API int sc_comm_init(const uint8_t *id128, int rank, int nranks, sc_comm **out);
SC_API int sc_comm_init_host(int rank, int nranks, sc_allreduce_u64_fn allreduce, sc_allgather_fn allgather, void *ctx, sc_comm **out);
/*   - or PEER TO PEER (sc_comm_init_p2p), for ranks that are THREADS of one process with one GPU each: no collective library at all.
 *     Every rank owns a fine-grained inbox on its device; the ranks meet under `group_id` (any number no other live group uses; the
 *     call blocks until all `nranks` threads have made it -- 60 s at most -- and enables peer access between their devices).  A round's
 *     all-reduce is then ONE small kernel per rank on the prover's stream: it pushes the rank's (deg+1) x 8 lanes into every peer's
 *     inbox as self-validating words (posted writes over xGMI), polls its own inbox, adds, and publishes the total to the host --
 *     instead of ncclAllReduce + a publishing kernel; the tail's gather is peer copies.  Ranks may share a GPU (functional tests on
 *     a one-GPU box; rounds are then not pipelined and the exchange kernel is re-launched until its peers' kernels have run).
 *     LIMITS: at most 16 ranks; round messages of at most 8 evaluations (max_multiplicands <= 7) -- sc_ml_prove_sharded returns
 *     SC_ERR_BAD_ARG for longer ones before it touches the handle.
 *     THREADS AND RCCL: an RCCL communicator driven by one thread per GPU inside one process must follow RCCL's own rule for that
 *     mode -- one communicator per thread, every thread issuing the same collectives in the same order, no thread holding a lock
 *     another needs while inside a collective.  The library's per-device gate is never held across devices, so distinct-device
 *     thread ranks satisfy it; one process per GPU (what bench.py launches) avoids the question, and sc_comm_init_p2p avoids RCCL. */
SC_API int sc_comm_init_p2p(uint64_t group_id, int rank, int nranks, sc_comm **out);
/* diagnostic, collective: one all-reduce and one all-gather of known patterns over the communicator, checked on every rank */
SC_API int sc_comm_selftest(sc_comm *comm);
SC_API void sc_comm_free(sc_comm *comm);
/* what the communicator itself knows: this rank, the number of ranks, and its kind (bench.py reports `ranks_seen` from here, not from
 * its command line) */
#define SC_COMM_RCCL 1
#define SC_COMM_HOST 2
#define SC_COMM_P2P 3
#define SC_COMM_DIRECT_PUBLISH 0x100 /* flag on SC_COMM_RCCL: the communicator's all-reduces deliver a round's (tagged) lanes straight into the
                                      * host-mapped page the host polls -- no publishing kernel behind them (probed by sc_comm_init; sc_set_policy("rccl_direct", 0)
                                      * switches it off) */
SC_API int sc_comm_info(sc_comm *comm, int *rank_out, int *nranks_out, int *kind_out);
/* measurement, collective (every rank calls it): `iters` back-to-back exchanges of n_words (<= 64) uint64 lanes in exactly the form a
 * sharded round uses on this communicator (RCCL: ncclAllReduce into the host-mapped page + the host's poll of the tagged words, or
 * ncclAllReduce + publishing kernel + poll where direct publication is unavailable; peer-to-peer: the one exchange
 * kernel + poll; host transport: publishing kernel + poll + the caller's all-reduce), each waited for before the next is issued; the
 * sums are checked.  *us_mean_out / *us_min_out_or_null: this rank's wall time per exchange.  The per-round cost a sharded proof pays
 * on top of its kernels (the reference's counterpart, the rayon reduce of prover.rs:139-148, is in-process). */
SC_API int sc_comm_exchange_bench(sc_comm *comm, uint32_t n_words, uint32_t iters, double *us_mean_out, double *us_min_out_or_null);
/* how long a host loop waits for a round's message or a peer's lanes before it gives the proof up (default 20 000 ms; also
 * SC_PUBLISH_TIMEOUT_MS in the environment; 0 restores the default).  Process-wide. */
SC_API int sc_set_publish_timeout_ms(uint32_t ms);
SC_API int sc_ml_prove_sharded(sc_prover *p, sc_comm *comm, sc_rng *rng_or_null, uint32_t nv_total, uint64_t *out_proof,
                               uint64_t *out_randomness);
SC_API int sc_ml_prove_sharded_rounds(sc_prover *p, sc_comm *comm, sc_rng *rng, uint32_t nv_total, uint32_t n_rounds, uint64_t *out_proof,
                                      uint64_t *out_randomness);

/* ---- DenseMultilinearExtension::fix_variables (ark-poly; prover.rs:88, gkr mod.rs:122) ------ */
/* in: 2^nv x 4 limbs, point: k x 4 limbs (binds variables 0..k-1, LSB first), out: 2^(nv-k) x 4.
 * flags: SC_TABLES_ON_DEVICE => `in` and `out` are device pointers. */
SC_API int sc_fix_variables(const uint64_t *in, uint32_t nv, const uint64_t *point, uint32_t k, uint64_t *out, uint32_t flags);

/* ---- Blake2b512Rng / FeedableRNG (reference src/rng.rs:11-81) -- host side ------------------- */
SC_API sc_rng *sc_rng_setup(void);
SC_API void sc_rng_free(sc_rng *rng);
SC_API void sc_rng_feed_bytes(sc_rng *rng, const uint8_t *buf, size_t len);             /* feed() after serialization */
SC_API void sc_rng_fill_bytes(sc_rng *rng, uint8_t *dest, size_t len);                  /* RngCore::fill_bytes */
SC_API void sc_rng_feed_poly_info(sc_rng *rng, uint64_t max_multiplicands, uint64_t num_variables); /* feed(&PolynomialInfo) */
SC_API void sc_rng_feed_prover_msg(sc_rng *rng, const uint64_t *evals, uint32_t n);     /* feed(&ProverMsg) */
SC_API void sc_rng_sample_fr(sc_rng *rng, uint64_t *out);                               /* sample_round = F::rand, verifier.rs:128-131 */

/* ---- MLSumcheck::prove / prove_as_subprotocol (reference src/ml_sumcheck/mod.rs:42-70) ------- */
/* rng_or_null: NULL = fresh Blake2b512Rng::setup() (MLSumcheck::prove).  out_proof: num_vars x (deg+1) x 4.
 * out_state_or_null: receives the ProverState handle (caller frees) as prove_as_subprotocol returns it.
 * The latency-bound late rounds do not go back to the host for their launches: rounds with more than 2048 pairs are pipelined (the
 * next round is enqueued behind a wait kernel before the current round's message is hashed), the last rounds (<= 2048 pairs) run in
 * ONE persistent kernel that publishes every message into host-mapped memory and polls a host-mapped mailbox for the challenge;
 * the calling thread only hashes and answers.  Every device-side wait is bounded (seconds); if the calling thread is stalled for
 * longer, messages computed on a stale challenge are never returned: a handle whose inputs are still there (borrowed or streamed
 * tables) proves again from round 0 with synchronous rounds inside the same call; otherwise the call returns SC_ERR_HIP ("... the
 * proof is void") -- reset the handle with its tables and prove again.  sc_set_policy("pipeline", 0) (or a runtime that serialises kernel launches, e.g. a counter-collecting
 * profiler, detected by a probe) turns all of it off: every round is then launched after its challenge is known. */
SC_API int sc_ml_prove(const sc_poly_desc *desc, sc_rng *rng_or_null, uint64_t *out_proof, sc_prover **out_state_or_null);
/* (One-shot use -- MLSumcheck::prove(&poly) in a loop -- does not pay for a prover per call: the library keeps the last one it built
 * here and rewinds it onto the next polynomial of the same structure; with out_state_or_null == NULL device tables are read in
 * place.  sc_release_caches gives the memory back.) */
/* n_rounds x (prove_round, feed, sample) of that loop (mod.rs:57-64) on a handle at round 0, continuing `rng` without feeding
 * PolynomialInfo: the last log2 G rounds of a sharded proof, on the gathered G-entry tables.  out_randomness: n_rounds x 4. */
SC_API int sc_ml_prove_rounds(sc_prover *p, sc_rng *rng, uint32_t n_rounds, uint64_t *out_proof, uint64_t *out_randomness);
/* the same loop on an existing handle at round 0 (sc_prover_init / sc_prover_reset): no allocation per proof */
SC_API int sc_ml_prove_handle(sc_prover *p, sc_rng *rng_or_null, uint64_t *out_proof);
/* n independent instances of MLSumcheck::prove (mod.rs:42-70), proved concurrently.  descs[i] are n complete descriptors of the
 * SAME structure (num_vars, max_multiplicands, n_products, prod_offsets, prod_indices, n_tables, flags); tables and coefficients
 * are per instance.  rngs_or_null: NULL = a fresh Blake2b512Rng::setup() per instance, else n transcripts, rngs[i] continued by
 * instance i exactly as sc_ml_prove continues its rng (PolynomialInfo fed first).  out_proofs: n x num_vars x (deg+1) x 4 limbs,
 * instance-major; out_randomness_or_null: n x num_vars x 4.  Instance i's output is bit for bit what
 * sc_ml_prove(&descs[i], rngs[i], ...) alone would have produced.  Caller memory is only read.
 * What a caller with many small instances (a GKR prover's side claims, a lookup argument per column, proofs for many clients) uses
 * instead of a loop -- the reference's caller would put a rayon par_iter around MLSumcheck::prove.  A whole proof over 2^6 .. 2^10
 * entries is latency from end to end; here every instance that fits ONE block's LDS (three tables up to 2^9 entries, two up to 2^10,
 * ten up to 2^8; products of at most 8 multiplicands) is proved by a block of its own, all of them in flight at once in one kernel
 * that publishes every message into host-mapped memory, while the calling thread hashes and answers whichever instance has
 * published.  The call is TOTAL over shapes: instances beyond that envelope, very small n, a busy device (another proof's persistent
 * kernel holds it) or device-side waits switched off take the serial plan -- instance after instance on one prover -- with the same
 * output; an instance whose block's bounded wait for the host expired is proved again by the serial plan inside the call
 * (sc_library_stats word 5 counts them).  Only argument errors return an error: n == 0 is SC_OK and touches nothing; the first
 * invalid instance decides the status (before any HIP call); a descriptor whose structure differs from descs[0] is SC_ERR_BAD_ARG
 * and sc_last_error() names the instance and the field.  Policy "batch" selects the plan.  Work areas are cached (sc_release_caches). */
SC_API int sc_ml_prove_batch(const sc_poly_desc *descs, uint32_t n, sc_rng *const *rngs_or_null, uint64_t *out_proofs,
                             uint64_t *out_randomness_or_null);
/* ---- n x IPForMLSumcheck::{prover_init, prove_round} (prover.rs:49-153) behind one handle: the interactive half of the batch ------
 * sc_ml_prove_batch keeps the crate's Blake2b transcript inside the call.  A caller with a transcript of its own -- the reference takes
 * fs_rng: &mut impl FeedableRNG: one transcript over all instances, one shared challenge per round, a hash on many threads -- proves n
 * small instances round by round here instead of looping sc_prove_round over n handles: the reference's caller would write
 * states.par_iter_mut().zip(msgs).map(prove_round).  Within sc_ml_prove_batch's envelope (every instance fits ONE block's LDS) a round of
 * the whole batch is one upload of the challenges, ONE kernel launch (a block per instance), one copy back and one synchronisation; every
 * challenge is known before the launch, so nothing on the GPU ever waits for the host (policies "pipeline" and "wait_spins" and the
 * device's tail slot play no part).  The calls are TOTAL over shapes: beyond the envelope, or with policy "batch" = 0 when the handle is
 * built, the handle holds n ordinary provers (device-side waits off, no resident kernel) and a round is a loop of sc_prove_round, with the
 * same bits; with policy "batch" = 1 or 2 the kernel runs for every n that fits.
 * SLICED ROUNDS [policy "batch_slices" = 1 when the handle is built; default 0]: shapes beyond one block's LDS keep the work area and the
 * per-round sequence -- 1 <= num_vars <= 16, products of at most eight multiplicands, a structure that travels as kernel arguments, a work
 * area [96 bytes x n x tables x 2^num_vars] of at most 16 GiB.  A round whose tables as loaded do not fit one block gives every instance to
 * several blocks, each a contiguous slice of every table [binding is LSB-first: a slice binds to a slice], as TWO plain launches -- the
 * slices' sums into a device array, then one block per instance that adds them and forms the message --; from the first round that fits,
 * the one-launch round above runs on the same work area.  Plan counters: batch.rounds_slices per sliced round call, batch.rounds_one_block
 * for the others.  State, bind_final, reset, push_randomness and every status code are the same for all three plans.  Measured against
 * the serial plan [tools/batch_round_slices_bench.py, profiles/batch_round_slices_bench.json]: ahead 9-12x at n = 16 and 26-138x at n = 256,
 * behind at n = 1 [0.77-0.87x]; the default stays 0.
 * THREADING: one handle, one host thread at a time; distinct handles are independent (the library serialises its HIP calls per device). */
typedef struct sc_batch_prover sc_batch_prover; /* n x ProverState (prover.rs:19-33) of ONE structure */
/* SC_API_EXT is SC_API.  It marks the entry points whose prototypes name an opaque type younger than the type table of the header-vs-shim
 * scanner in tests/test_rust_shim.py (which reads `SC_API` prototypes and cannot map sc_batch_prover); tests/test_batch_rounds_host.py
 * compares these prototypes with the shim's declarations instead, with the same rules. */
#define SC_API_EXT SC_API
/* descs: n complete descriptors of the SAME structure -- sc_ml_prove_batch's rule, check and error text ("instance %u: ...").  Everything
 * the host can check is checked before any HIP call, so an argument error is the same with or without a GPU: num_vars == 0 is
 * SC_ERR_CONSTANT_POLY, n == 0 is SC_ERR_BAD_ARG (a handle over nothing is not a handle), a non-canonical coefficient SC_ERR_BAD_ARG.
 * Tables are host or device memory per descs[0].flags and are COPIED, as sc_prover_init copies (device tables after a device-wide
 * synchronise): nothing of the caller's is read after the call returns.  SC_TABLES_BORROW, SC_TABLES_STREAM and SC_NO_DEVICE_POLLING are
 * ignored.  Device memory: 96 bytes per table entry (every binding depth keeps its own region, so the round-0 tables survive the proof)
 * plus, for host tables, the 32-byte staging copy a reset with new tables reuses. */
SC_API_EXT int sc_batch_prover_init(const sc_poly_desc *descs, uint32_t n, sc_batch_prover **out);
/* One prove_round (prover.rs:74-153) for every instance.  r_or_null: NULL exactly on the first call; afterwards the previous round's
 * challenges, n x 4 limbs instance-major, or -- r_shared != 0 -- 4 limbs for all instances.  out_evals: n x (max_multiplicands+1) x 4
 * limbs, instance-major.  Instance i's message is bit for bit what sc_prove_round on a handle over descs[i] returns for the same
 * challenges.  Misuse maps to sc_prove_round's status codes: SC_ERR_FIRST_ROUND_HAS_MSG, SC_ERR_MISSING_MSG, SC_ERR_NOT_ACTIVE after
 * num_vars rounds; a non-canonical challenge is SC_ERR_BAD_ARG "instance %u: challenge is not canonical".  An argument error leaves
 * the handle exactly where it was. */
SC_API_EXT int sc_batch_prove_round(sc_batch_prover *bp, const uint64_t *r_or_null, uint32_t r_shared, uint64_t *out_evals);
/* MLSumcheck::prove_as_subprotocol pushes the final challenge without binding it (mod.rs:65-67): r as for sc_batch_prove_round. */
SC_API_EXT int sc_batch_prover_push_randomness(sc_batch_prover *bp, const uint64_t *r, uint32_t r_shared);
/* sc_prover_state for ONE instance of the batch.  randomness: up to num_vars x 4 limbs (may be NULL); tables_out: U x 2^(num_vars - bound)
 * x 4 limbs of canonical elements, bound = max(round-1, 0) (may be NULL); *round, *n_randomness may be NULL. */
SC_API_EXT int sc_batch_prover_state(sc_batch_prover *bp, uint32_t instance, uint64_t *randomness, uint32_t *n_randomness, uint64_t *tables_out,
                                 uint32_t *round);
/* sc_prover_bind_final for the batch: after the last round, bind the last variable of every instance's tables with its challenge (r as
 * for sc_batch_prove_round).  out_table_values: n x U x 4 limbs on the HOST -- the table evaluations at each instance's point, bit for bit
 * the out_table_values of sc_poly_evaluate there.  Afterwards the handle is exhausted until it is reset. */
SC_API_EXT int sc_batch_prover_bind_final(sc_batch_prover *bp, const uint64_t *r, uint32_t r_shared, uint64_t *out_table_values);
/* Rewind the handle to round 0 without reallocating.  descs_or_null == NULL: the tables copied by init (or by the last reset) again --
 * the handle keeps them; otherwise n new descriptors of the handle's structure, copied in as by init (new tables, new coefficients; a
 * handle built over device tables takes device tables). */
SC_API_EXT int sc_batch_prover_reset(sc_batch_prover *bp, const sc_poly_desc *descs_or_null);
SC_API_EXT void sc_batch_prover_free(sc_batch_prover *bp);

/* ---- verifier (reference src/ml_sumcheck/protocol/verifier.rs:90-251) -- host side, O(nv*deg) - */
/* interpolate_uni_poly (verifier.rs:139-251, including its three tiers: i64 ratios for len <= 20, i128 for len <= 33, field
 * elements beyond).  Every input element must be canonical (< p), else SC_ERR_BAD_ARG. */
SC_API int sc_interpolate_uni_poly(const uint64_t *p_i, uint32_t len, const uint64_t *eval_at, uint64_t *out);
/* MLSumcheck::verify_as_subprotocol (mod.rs:84-100): returns SC_OK / SC_ERR_REJECT;
 * proof: num_vars x (max_multiplicands+1) x 4 limbs; proof_elems: the number of field elements the caller's buffer holds --
 * anything but num_vars * (max_multiplicands+1) is SC_ERR_BAD_ARG "incorrect number of evaluations" (verifier.rs:60-62), so
 * the library never reads past it.  claimed_sum and every proof element must be canonical (< p): the reference's Fp cannot
 * hold anything else, and a non-canonical encoding is rejected with SC_ERR_BAD_ARG before any arithmetic.
 * out_point: num_vars x 4, out_expected: 4 limbs (SubClaim, verifier.rs:29-34). */
SC_API int sc_ml_verify(uint32_t num_vars, uint32_t max_multiplicands, const uint64_t *claimed_sum, const uint64_t *proof,
                 uint64_t proof_elems, sc_rng *rng_or_null, uint64_t *out_point, uint64_t *out_expected);

/* ---- GKR round sumcheck (reference src/gkr_round_sumcheck/mod.rs) ---------------------------- */
/* f1 is a SparseMultilinearExtension over 3*dim variables given as nnz (index, value) pairs with
 * distinct indices (index layout z | x<<dim | y<<2dim, mod.rs:34-35); g / u are host arrays (dim x 4 limbs).
 * flags: SC_TABLES_ON_DEVICE => every table-sized argument (f1_idx, f1_vals, f2, f3 and, for the two initialisation
 * calls, the outputs h_g, f1g_idx, f1g_vals, f1_gu) is a DEVICE pointer: inputs are read in place (never written), outputs
 * are produced in place; without it they are host arrays that the call stages through HBM.  The proof itself, u, v and
 * *f1g_nnz always land on the host.
 * initialize_phase_one (mod.rs:22-42): h_g = 2^dim x 4 out; f1_g out as sorted (index,value) pairs,
 * capacity nnz, *f1g_nnz = count.  A list that arrives in index order (what iterating a BTreeMap gives) is not sorted again;
 * the dense table is accumulated from the list as it came. */
SC_API int sc_gkr_phase_one(const uint64_t *f1_idx, const uint64_t *f1_vals, uint64_t nnz, uint32_t dim, const uint64_t *f3,
                     const uint64_t *g, uint32_t flags, uint64_t *h_g, uint64_t *f1g_idx, uint64_t *f1g_vals, uint64_t *f1g_nnz);
/* initialize_phase_two (mod.rs:57-63): f1_gu = 2^dim x 4 out.  Any order of the list; repeated indices add up. */
SC_API int sc_gkr_phase_two(const uint64_t *f1g_idx, const uint64_t *f1g_vals, uint64_t nnz, uint32_t dim, const uint64_t *u,
                     uint32_t flags, uint64_t *f1_gu);
/* GKRRoundSumcheck::prove (mod.rs:93-139).  out_proof: 2 x dim x 3 x 4 limbs (phase1 then phase2
 * messages); out_uv_or_null: 2 x dim x 4 (u then v).
 * The proof needs the two dense tables of the initialisations but not f1(g,.,.) as a list, so this entry point does not sort: the
 * non-zeros' terms are grouped by target cell and added up in LDS (exact field sums in any order give the reference's bits); repeated
 * indices are summed, as a map built by insertion-with-add would; an index-ordered list (BTreeMap order) saves one grouping pass.
 * sc_gkr_phase_one / _two above return the list and take the sorting route. */
SC_API int sc_gkr_prove(sc_rng *rng, const uint64_t *f1_idx, const uint64_t *f1_vals, uint64_t nnz, uint32_t dim,
                 const uint64_t *f2, const uint64_t *f3, const uint64_t *g, uint32_t flags, uint64_t *out_proof, uint64_t *out_uv_or_null);
/* n independent instances of GKRRoundSumcheck::prove (mod.rs:93-139) of one `dim`, proved concurrently.
 * Per instance i: f1_idx[i] / f1_vals[i] (nnz[i] pairs), f2[i], f3[i] (2^dim x 4 limbs), g[i] (dim x 4, host).
 * Pointers may repeat across instances (one wiring predicate f1 for many data instances is the usual case).
 * flags: SC_TABLES_ON_DEVICE => f1_idx[i], f1_vals[i], f2[i], f3[i] are device pointers, read in place;
 * the pointer arrays themselves, nnz[] and g[i] are always host memory.
 * rngs: n transcripts, all distinct, rngs[i] continued exactly as sc_gkr_prove continues its rng.
 * out_proofs: n x 2 x dim x 3 x 4 limbs, instance-major; out_uv_or_null: n x 2 x dim x 4.
 * Instance i's proof, (u, v) and the final state of rngs[i] are bit for bit what sc_gkr_prove on rngs[i] alone would have produced
 * (repeated indices summed, any order of the list, zero values).  Small instances -- dim <= 9 and nnz[i] <= 64 x 2^dim for every i:
 * both tables of a phase, the two eq tables and the cells the non-zeros are added into within one workgroup's LDS -- are proved a
 * workgroup each inside one kernel, the host hashing and answering; every other shape runs instance after instance through
 * sc_gkr_prove's path inside the call, with the same bits.  Policy "batch" selects the plan as for sc_ml_prove_batch.
 * The argument checks are sc_gkr_prove's, per instance; everything the host can check is checked before any HIP call, so a bad
 * argument is SC_ERR_BAD_ARG with or without a GPU.  The lowest failing instance decides the status, sc_last_error() starts with
 * "instance %u: ", and no caller transcript has been advanced when an argument error is returned (an out-of-range index in a
 * device-resident list included: it is found on the device in front of the proofs, never followed).  n == 0: SC_OK, nothing is touched.
 * A null rngs[i], or one sc_rng twice: SC_ERR_BAD_ARG.  dim == 0: SC_ERR_CONSTANT_POLY.  Work areas are cached (sc_release_caches). */
SC_API int sc_gkr_prove_batch(uint32_t n, uint32_t dim, sc_rng *const *rngs,
                              const uint64_t *const *f1_idx, const uint64_t *const *f1_vals, const uint64_t *nnz,
                              const uint64_t *const *f2, const uint64_t *const *f3, const uint64_t *const *g,
                              uint32_t flags, uint64_t *out_proofs, uint64_t *out_uv_or_null);
/* ---- n x the interactive rounds of GKRRoundSumcheck::prove (mod.rs:93-139) behind one handle, under the caller's transcript ----------
 * sc_gkr_prove_batch keeps the crate's Blake2b transcript inside the call, one per instance.  GKRRoundSumcheck::prove is where the
 * reference most plainly takes rng: &mut impl FeedableRNG: a GKR prover runs one round sumcheck per layer or per copy of a sub-circuit
 * under ONE transcript, often with one challenge per round for all of them.  This family is to sc_gkr_prove_batch what sc_batch_prover_*
 * is to sc_ml_prove_batch: the caller hashes (on as many threads as it likes) and hands in every challenge; a proof is 2 x dim round
 * calls -- phase one's dim messages, then phase two's -- and one call of sc_gkr_batch_prover_finish.  Within sc_gkr_prove_batch's envelope
 * [dim <= 9, nnz <= 64 x 2^dim] a round call is one upload of the challenges, ONE kernel launch [a block per instance; the call that
 * starts phase two: two launches back to back], one copy back and one synchronisation, and nothing on the GPU ever waits for the host.
 * The calls are TOTAL over shapes: beyond the envelope, or with policy "batch" = 0 when the handle is built, the handle holds per
 * instance what sc_gkr_prove's path holds [the two dense tables by its route, an ordinary prover per phase, device-side waits off] and
 * a round is a loop of sc_prove_round, with the same bits.
 * DIM 10 .. 16 [policy "batch_slices" = 1 when the handle is built; default 0; nnz <= 64 x 2^dim; two work areas and the accumulator cells,
 * 448 B x 2^dim per instance, at most 16 GiB]: plan batch.gkr_rounds_slices keeps the work areas and the per-call sequence; each of the two
 * initialisations is a memset and two launches that give an instance to many blocks [the terms are added into wide integer cells in device
 * memory: exact in any order, the same bits], and for dim >= 11 rounds 0 .. dim - 10 of each phase are the two launches of the sliced rounds
 * above.  Counted once per round call, 2 x dim per proof; state, finish, reset, the shared challenge and every status are unchanged.
 * THREADING: as for sc_batch_prover_*. */
typedef struct sc_gkr_batch_prover sc_gkr_batch_prover;   /* n x the two ProverStates of GKRRoundSumcheck::prove (mod.rs:93-139), one dim */
/* SC_API_GKRB is SC_API: the marker of this family, for the reason SC_API_EXT has one [tests/test_gkr_batch_rounds_host.py compares
 * these prototypes with the shim's declarations]. */
#define SC_API_GKRB SC_API /* [nothing but this comment may follow on the line] */
/* Arguments, meaning and checks are sc_gkr_prove_batch's, without the rngs [pointers may repeat across instances; SC_TABLES_ON_DEVICE as
 * there; g[i] is host memory].  Everything the host can check is checked before any HIP call: errors start with "instance %u: ", the
 * lowest failing instance decides; n == 0 is SC_ERR_BAD_ARG, dim == 0 SC_ERR_CONSTANT_POLY.  An out-of-range index in a device-resident
 * list is found on the device in front of any kernel that follows the indices [SC_ERR_BAD_ARG "instance %u: f1 has an index out of
 * range"].  Every input is COPIED, once per distinct pointer: nothing of the caller's is read after the call returns.  The plan is chosen
 * here, from policy "batch", policy "batch_slices", dim and the largest nnz [batch.gkr_rounds_one_block: dim <= 9; batch.gkr_rounds_slices:
 * dim 10 .. 16 under "batch_slices" = 1; batch.gkr_rounds_serial: everything else], and phase one's tables are built before the call returns. */
SC_API_GKRB int sc_gkr_batch_prover_init(uint32_t n, uint32_t dim, const uint64_t *const *f1_idx, const uint64_t *const *f1_vals, const uint64_t *nnz,
                                         const uint64_t *const *f2, const uint64_t *const *f3, const uint64_t *const *g, uint32_t flags,
                                         sc_gkr_batch_prover **out);
/* Called 2 x dim times: call t < dim returns phase one's message t of every instance, call dim .. 2 dim - 1 phase two's.  r_or_null: NULL
 * exactly on call 0; afterwards the previous round's challenges, n x 4 limbs instance-major, or -- r_shared != 0 -- 4 limbs for all
 * instances [the challenge handed to call dim is u_{dim-1}].  out_evals: n x 3 x 4 limbs.  Instance i's 2 x dim messages are bit for bit
 * what GKRRoundSumcheck::prove computes for the same challenges.  Misuse maps to sc_batch_prove_round's status codes:
 * SC_ERR_FIRST_ROUND_HAS_MSG, SC_ERR_MISSING_MSG, SC_ERR_NOT_ACTIVE after 2 x dim rounds; a non-canonical challenge is SC_ERR_BAD_ARG
 * "instance %u: challenge is not canonical".  An argument error leaves the handle exactly where it was. */
SC_API_GKRB int sc_gkr_batch_prove_round(sc_gkr_batch_prover *bp, const uint64_t *r_or_null, uint32_t r_shared, uint64_t *out_evals);
/* After 2 x dim rounds: takes the last challenge v_{dim-1} [r as above].  out_uv_or_null: n x 2 x dim x 4 limbs in sc_gkr_prove_batch's
 * layout [a shared challenge is expanded]; out_final_or_null: n x 3 x 4 limbs -- f1(g,u,v), f2(u), f2(u) f3(v): phase two's two tables
 * bound to one entry and the scalar from the phase change, so the subclaim's oracle queries cost no extra pass; the product of the first
 * and the third is what the verifier compares with its expected evaluation.  Afterwards the handle is exhausted until it is reset. */
SC_API_GKRB int sc_gkr_batch_prover_finish(sc_gkr_batch_prover *bp, const uint64_t *r, uint32_t r_shared, uint64_t *out_uv_or_null, uint64_t *out_final_or_null);
/* sc_batch_prover_state's job for ONE instance.  *round: 0 .. 2 dim; randomness: u followed by the v's received so far [up to 2 dim x 4
 * limbs]; tables_out: the current phase's two tables, 2 x 2^(dim - bound) canonical elements, bound = max(the phase's round - 1, 0) --
 * phase one's until call dim has been answered.  Every pointer but bp may be NULL. */
SC_API_GKRB int sc_gkr_batch_prover_state(sc_gkr_batch_prover *bp, uint32_t instance, uint64_t *randomness, uint32_t *n_randomness,
                                          uint64_t *tables_out, uint32_t *round);
/* Rewind to round 0 over the inputs the handle holds, without reallocating and without rebuilding phase one's tables.  New inputs:
 * sc_gkr_layer_next_batch, below. */
SC_API_GKRB int sc_gkr_batch_prover_reset(sc_gkr_batch_prover *bp);
SC_API_GKRB void sc_gkr_batch_prover_free(sc_gkr_batch_prover *bp);
/* ---- the handle onto the NEXT LAYER's inputs, without a rebuild ---------------------------------------------------------------------------
 * A GKR prover runs one round sumcheck per layer under one transcript, and every layer has new inputs: its g is the previous layer's
 * point [the output layer's; a layer below it starts from TWO points: sc_gkr_two_point_next_batch, further down], its f2 and f3 are the
 * next layer's values, often it has wiring of its own.  sc_gkr_layer_next_batch puts an existing handle onto
 * them: it ALLOCATES NOTHING and leaves the handle at round 0 with phase one's tables built, exactly as a fresh sc_gkr_batch_prover_init
 * over these inputs would -- same plan, same bits.  It may be called in any state [fresh, in the middle of either phase, after finish];
 * afterwards round is 0, the kept randomness is empty and the handle is not exhausted.
 * SC_API_GKRL is SC_API: a marker of its own, for the reason SC_API_EXT and SC_API_GKRB have one [tests/test_gkr_next_layer_host.py
 * compares this prototype with the shim's declaration; the older scanners each assert a closed set]. */
#define SC_API_GKRL SC_API /* [nothing but this comment may follow on the line] */
/* Arguments mean what they mean for sc_gkr_batch_prover_init; n and dim are the handle's.  flags & SC_TABLES_ON_DEVICE must equal what the
 * handle was built with [SC_ERR_BAD_ARG otherwise].  f1: all three of f1_idx, f1_vals and nnz NULL keeps the wiring the handle holds, all
 * three given is new wiring, a mixture is SC_ERR_BAD_ARG.  f2, f3 and g are required; pointers may repeat within and across instances.
 * PLAN: the one chosen at init.  New wiring that a handle with work areas would not have been built for [an nnz above 64 x 2^dim] is
 * SC_ERR_BAD_ARG naming the instance; a handle on the serial plan takes every shape and stays serial.
 * CAPACITY: the handle's copy of the inputs is laid out again by init's rule, every distinct [pointer, size] once, inside the bytes
 * reserved at init; with kept wiring the wiring's arrays stay where they are and the distinct f2 / f3 take the places the former ones had.
 * A layout that does not fit is SC_ERR_BAD_ARG with both byte counts and "build a new handle".  A call ALWAYS fits if its pointers repeat
 * in the same pattern as init's and its f1 is kept or has nnz[i] <= init's nnz[i] for every i.  Init reserves no slack for growth.
 * ERRORS: every check the host can make runs before any HIP call; the lowest failing instance decides, errors start with "instance %u: "
 * [init's own per-instance checks, a non-canonical g].  An out-of-range index in a device-resident list is found on the device, over the
 * caller's arrays, before anything of the handle's is overwritten [SC_ERR_BAD_ARG "instance %u: f1 has an index out of range"].  ANY of
 * these errors leaves the handle exactly where it was: a proof in progress continues with the same bits.  [A HIP error later in the call
 * leaves the handle exhausted and its inputs undefined until the next successful call of this function.]
 * SYNCHRONOUS: device inputs are read after a device-wide synchronise, as at init; nothing of the caller's is read after the call returns.
 * Device arrays come in through ONE kernel launch for all of them [k_batch_gkr_restage], host arrays by init's copies.  Counted as plan
 * batch.gkr_next_layer, once per successful call on a handle with work areas. */
SC_API_GKRL int sc_gkr_layer_next_batch(sc_gkr_batch_prover *bp, const uint64_t *const *f1_idx_or_null, const uint64_t *const *f1_vals_or_null,
                                        const uint64_t *nnz_or_null, const uint64_t *const *f2, const uint64_t *const *f3, const uint64_t *const *g,
                                        uint32_t flags);
/* ---- the TWO-POINT form of the handle: a layer whose claim stands at two points -------------------------------------------------------------
 * GKRRoundSumcheck::verify ends a round with a subclaim at TWO points, u and v [mod.rs:183-191; data_structures.rs:33-56]; the next layer's
 * values W are claimed at W[u] and at W[v].  Only the output layer's g is one point.  Every layer below it starts from a linear
 * combination of two claims [XZZPS19, the paper the reference module cites], proved by one round sumcheck:
 *     alpha W[g] + beta W[g2]  =  sum over x, y of [ alpha f1[g,x,y] + beta f1[g2,x,y] ] f2[x] f3[y].
 * Per instance i the caller gives, besides sc_gkr_batch_prover_init's arguments, a second point g2[i] [dim x 4 limbs, host] and two
 * coefficients coef[i] = [alpha_i, beta_i] [coef: n x 2 x 4 limbs, instance-major, host, Montgomery, canonical].  Wherever the handle
 * uses eq[g_i, z] it uses E_i[z] = alpha_i eq[g_i, z] + beta_i eq[g2_i, z] instead: phase one's h[x] = sum E[z] v f3[y], phase two's
 * f1_gu[y] = sum E[z] eq[u,x] v.  Rounds, the phase change, f2[u], finish, state, reset, the shared challenge and every status are
 * untouched; finish's first value is alpha f1[g,u,v] + beta f1[g2,u,v].  Every output is a canonical field element: the three plans give
 * the same bits.  [alpha, beta] = [1, 0], beta = 0, alpha = beta = 0 and g2 = g are ordinary inputs; [1, 0] gives the one-point bits.
 * EVERY handle can change form layer by layer: both inits reserve room for g2 and coef [n x [dim + 2] x 32 bytes in the upload area and
 * in a layer's staging image; the input area's accounting, in_cap and the capacity error's byte counts do not move];
 * sc_gkr_layer_next_batch on a handle in two-point form returns it to the one-point form, sc_gkr_two_point_next_batch works on a handle
 * built by either init, sc_gkr_batch_prover_reset keeps the form.
 * PLANS: one block per instance [dim <= 9] builds eq[g2, .] in the LDS region eq[u, .] will occupy and folds it into eq[g, .] in one pass
 * -- no LDS beyond 128 B x 2^dim; the sliced plan keeps a second pair of half tables with alpha and beta folded into the low halves -- one
 * fr_mul and one fr_add more per term, the lanes' bound unchanged; the serial plan combines the dense tables of g and of g2 by linearity.
 * Counted as plan batch.gkr_two_point, once per successful call of either function below, on any plan.
 * SC_API_GKR2 is SC_API; a marker of its own, for the reason the older families have theirs [tests/test_gkr_two_point_host.py compares
 * these prototypes with the shim's declarations; every older scanner asserts a closed set]. */
#define SC_API_GKR2 SC_API /* [nothing but this comment may follow on the line] */
/* sc_gkr_batch_prover_init with g2 and coef; the same checks before any HIP call, and behind them per instance: a null g2[i] is
 * SC_ERR_BAD_ARG "instance %u: null argument", then "instance %u: g2 is not canonical", then "instance %u: coefficient is not canonical".
 * A null g2 or coef is SC_ERR_BAD_ARG "null argument".  The lowest failing instance decides. */
SC_API_GKR2 int sc_gkr_two_point_init_batch(uint32_t n, uint32_t dim, const uint64_t *const *f1_idx, const uint64_t *const *f1_vals, const uint64_t *nnz,
                                            const uint64_t *const *f2, const uint64_t *const *f3, const uint64_t *const *g, const uint64_t *const *g2,
                                            const uint64_t *coef, uint32_t flags, sc_gkr_batch_prover **out);
/* sc_gkr_layer_next_batch with g2 and coef, which are checked with g and staged where g is staged; every error of that call and the three
 * above leave a proof in progress exactly where it was: nothing of the handle's is written before the last check has passed. */
SC_API_GKR2 int sc_gkr_two_point_next_batch(sc_gkr_batch_prover *bp, const uint64_t *const *f1_idx_or_null, const uint64_t *const *f1_vals_or_null,
                                            const uint64_t *nnz_or_null, const uint64_t *const *f2, const uint64_t *const *f3, const uint64_t *const *g,
                                            const uint64_t *const *g2, const uint64_t *coef, uint32_t flags);
/* ---- the values of a circuit's layers: what every call above consumes as f2 and f3 -------------------------------------------------------
 * The prover's f2 and f3 for a layer are the values W of the layer underneath ["the next layer's values"].  This call computes them, for n
 * instances of one dim and n_layers layers, on the device:
 *     L[f1, A, B][z] = sum over f1's non-zeros [z | x << dim | y << 2 dim, v] of  v A[x] B[y]
 *     out[0 n + i] = L[f1[0 n + i], f2[i], f3[i]]                    layer 0 is the one next to the inputs
 *     out[k n + i] = L[f1[k n + i], out[[k-1] n + i], out[[k-1] n + i]]   k >= 1: a layer reads the layer before it on both sides
 * n_layers == 1 is the plain single-layer evaluation with independent f2 and f3.  Index layout, masking, "repeated indices add up", "any
 * order of the list" and "zero values are ordinary" are exactly sc_gkr_prove's; outputs are canonical Montgomery limbs, 2^dim x 4 each.
 * f1_idx, f1_vals, nnz and out are n_layers x n arrays, layer-major; f2 and f3 are n arrays.  Pointers may repeat across instances and across
 * layers [one wiring for all instances is the usual case]; the pointer arrays and nnz[] are always host memory.  flags: SC_TABLES_ON_DEVICE
 * => every list, table and output is a device pointer, inputs are read in place and outputs are written in place -- out[k] is then usable
 * directly as f2 / f3 of sc_gkr_batch_prover_init and sc_gkr_layer_next_batch; without it they are host arrays staged through a cached
 * work area [sc_release_caches frees it].  The call is synchronous, as the handle's init is.
 * CHECKS, all before any HIP call where the host can make them; the lowest failing [layer, instance] decides and sc_last_error() starts
 * with "layer %u instance %u: ": n == 0 or n_layers == 0 is SC_OK and touches nothing; a null argument is SC_ERR_BAD_ARG; dim == 0 is
 * SC_ERR_CONSTANT_POLY; dim > 21 is SC_ERR_BAD_ARG; per [layer, instance] nnz >= 2^31 [a lane of a cell must stay below 2^63], a null
 * entry, an output range that overlaps another output or any input, a host-resident index with a bit at or above 3 dim ["... f1 has an
 * index out of range"] are SC_ERR_BAD_ARG.  A device-resident list with such an index is found on the device, over all layers, in front of
 * the first launch that follows indices [same status and text]: no output has been written then.
 * PLANS, counted once per successful call, same bits: batch.gkr_eval_layers_one_block [dim <= 9 and every nnz <= 64 x 2^dim, policy "batch"
 * != 0]: ONE launch for all layers, one block per instance, tables and cells in 128 B x 2^dim of LDS; batch.gkr_eval_cells [every other
 * shape]: per layer the cells zeroed, a terms launch [integer atomics into 64 B x n x 2^dim of device memory from the cached work area; a
 * request above 16 GiB is SC_ERR_OOM with the byte count] and a fold launch on one stream.
 * SC_API_GKRE is SC_API; a marker of its own, for the reason the older families have theirs [tests/test_gkr_layers_eval_host.py compares
 * the prototype with the shim's declaration; every older scanner asserts a closed set]. */
#define SC_API_GKRE SC_API /* [nothing but this comment may follow on the line] */
/* f1_idx, f1_vals, nnz, out: n_layers x n, layer-major; f2, f3: n, layer 0's inputs; out: each 2^dim x 4 limbs. */
SC_API_GKRE int sc_gkr_layers_eval_batch(uint32_t n, uint32_t dim, uint32_t n_layers, const uint64_t *const *f1_idx, const uint64_t *const *f1_vals,
                                         const uint64_t *nnz, const uint64_t *const *f2, const uint64_t *const *f3, uint32_t flags, uint64_t *const *out);
/* ---- the GATE form of the handle: layers of multiplication AND addition gates -----------------------------------------------------------------
 * Every layer the calls above prove is a sum of multiplication gates.  XZZPS19 [the paper the two-point form follows] proves layers of both
 * kinds of gate, two wiring lists per layer:
 *     W_out[z] = sum over MUL [z,x,y,v] of  v f2[x] f3[y]   +   sum over ADD [z,x,y,v] of  v [f2[x] + f3[y]].
 * With E[z] = eq[g,z], or alpha eq[g,z] + beta eq[g2,z] in two-point form, the claim E-weighted over z is proved by two sumchecks of one shape:
 *     phase one over x:  f2[x] H1[x] + H2[x],   H1[x] = sum_MUL E[z] v f3[y] + sum_ADD E[z] v,   H2[x] = sum_ADD E[z] v f3[y];
 *     phase two over y:  f3[y] T1[y] + T2[y],   T1[y] = f2[u] sum_MUL E[z] eq[u,x] v + sum_ADD E[z] eq[u,x] v,   T2[y] = f2[u] sum_ADD E[z] eq[u,x] v.
 * Messages are three evaluations at 0, 1, 2, as before: n x 3 x 4 limbs per round call, 2 x dim round calls per layer.  P_0[0] + P_0[1] is
 * alpha W_out[g] + beta W_out[g2]; phase one's last message at u_last is phase two's claim; phase two's last message at v_last is
 * M f2[u] f3[v] + A [f2[u] + f3[v]] with M and A the E-weighted extensions of the two lists at [u, v].  Every message is the field sum of the
 * messages of the three multiplication-only instances [MUL, f2, f3], [ADD, f2, 1], [ADD, 1, f3] under the same challenges.
 * A handle built by sc_gkr_gates_init_batch is a sc_gkr_batch_prover: sc_gkr_batch_prove_round, _finish, _reset, _state and _free work on it
 * with the calling convention and status codes they have.  On this form
 *     finish's out_final is  f2[u], f3[v], f3[v] T1[v] + T2[v]  -- the THIRD value is what the verifier compares with its expected evaluation;
 *     state returns the round and the randomness; a non-NULL tables_out is SC_ERR_BAD_ARG [the plans hold different tables];
 *     sc_gkr_layer_next_batch and sc_gkr_two_point_next_batch refuse the handle with SC_ERR_BAD_ARG, and sc_gkr_gates_next_batch refuses a
 *     handle of the older inits.
 * PLANS, chosen at init, same bits [every output is a canonical element]: batch.gkr_gates_one_block -- dim <= 9, each list <= 64 x 2^dim,
 * policy "batch" != 0 and policy "gkr_gates_fused" = 1 [the default; read at init]: one block per instance fills work areas of three
 * tables [k_batch_gkr_gates_phase, two passes over one array of cells inside 128 B x 2^dim of LDS], the rounds are the batch handle's
 * round kernel over three tables and two products; batch.gkr_gates_composed -- every other shape up to dim 21: an inner handle of 3 n
 * multiplication-only instances on whatever plan IT chooses [one block, "batch_slices", serial], challenges replicated, the three messages
 * added on the host.  Each is counted once per round call.
 * SC_API_GKRG is SC_API; a marker of its own, for the reason the older families have theirs [tests/test_gkr_gates_host.py compares these
 * prototypes with the shim's declarations; every older scanner asserts a closed set]. */
#define SC_API_GKRG SC_API /* [nothing but this comment may follow on the line] */
/* sc_gkr_two_point_init_batch with two lists.  Argument meaning, SC_TABLES_ON_DEVICE, "copied once per distinct pointer" and the checks with
 * their order are that call's; each list is checked as f1 is there and an error names the list ["instance %u: mul index %llu out of range"
 * for a host list, "instance %u: mul has an index out of range" / "instance %u: add has an index out of range" for a device list].  A list
 * with nnz == 0 may have null pointers.  g2_or_null and coef_or_null both NULL: one point; both given: two points; a mixture is
 * SC_ERR_BAD_ARG. */
SC_API_GKRG int sc_gkr_gates_init_batch(uint32_t n, uint32_t dim, const uint64_t *const *mul_idx, const uint64_t *const *mul_vals, const uint64_t *mul_nnz,
                                        const uint64_t *const *add_idx, const uint64_t *const *add_vals, const uint64_t *add_nnz, const uint64_t *const *f2,
                                        const uint64_t *const *f3, const uint64_t *const *g, const uint64_t *const *g2_or_null, const uint64_t *coef_or_null,
                                        uint32_t flags, sc_gkr_batch_prover **out);
/* sc_gkr_two_point_next_batch for a gate handle [g2_or_null and coef_or_null as at init: the layer's form].  The six wiring arguments are all
 * NULL [both lists are kept] or all given; anything else is SC_ERR_BAD_ARG.  The plan is init's; on batch.gkr_gates_one_block a new list
 * above 64 x 2^dim is SC_ERR_BAD_ARG naming the instance and the list.  CAPACITY: the handle's copy of the inputs is laid out again by
 * init's rule -- the lists at the front, f2 / f3 behind them, every distinct [pointer, size] once -- inside the bytes init reserved; kept
 * wiring stays where it is.  A call always fits if its pointers repeat in init's pattern and its lists are kept or no longer than init's.  Every check -- the host's, the capacity rule, the
 * index check of new device-resident lists over the caller's arrays -- comes before the first write: ANY such error leaves the proof in
 * progress exactly where it was.  [A HIP error later leaves the handle exhausted until the next successful call.] */
SC_API_GKRG int sc_gkr_gates_next_batch(sc_gkr_batch_prover *bp, const uint64_t *const *mul_idx_or_null, const uint64_t *const *mul_vals_or_null,
                                        const uint64_t *mul_nnz_or_null, const uint64_t *const *add_idx_or_null, const uint64_t *const *add_vals_or_null,
                                        const uint64_t *add_nnz_or_null, const uint64_t *const *f2, const uint64_t *const *f3, const uint64_t *const *g,
                                        const uint64_t *const *g2_or_null, const uint64_t *coef_or_null, uint32_t flags);
/* sc_gkr_layers_eval_batch with both lists per [layer, instance]: out = L[mul, A, B] + sum over add's non-zeros [z | x << dim | y << 2 dim, v]
 * of v [A[x] + B[y]], [A, B] = [f2, f3] for layer 0 and the layer before on both sides afterwards -- what sc_gkr_gates_init_batch and
 * sc_gkr_gates_next_batch consume as f2 and f3.  mul_* and add_*: n_layers x n arrays, layer-major; a list with nnz == 0 may have null
 * pointers.  Every check of that call holds, the overlap check included [the ADD lists are inputs as the MUL lists are]; an index error names
 * the list ["layer %u instance %u: mul has an index out of range" / "... add has an index out of range"], a device-resident one is found
 * over all layers before any output is written.  The condition on the lanes applies to the two lists together: mul_nnz + add_nnz < 2^31
 * per [layer, instance].  PLANS, counted once per successful call, same bits: batch.gkr_gates_eval_one_block [dim <= 9, every list of either
 * kind <= 64 x 2^dim, policy "batch" != 0: ONE launch for all layers, both lists into the same cells in LDS] and batch.gkr_gates_eval_cells
 * [every other shape: per layer the cells zeroed, a terms launch per kind of list, a fold launch]. */
SC_API_GKRG int sc_gkr_gates_layers_eval_batch(uint32_t n, uint32_t dim, uint32_t n_layers, const uint64_t *const *mul_idx, const uint64_t *const *mul_vals,
                                               const uint64_t *mul_nnz, const uint64_t *const *add_idx, const uint64_t *const *add_vals, const uint64_t *add_nnz,
                                               const uint64_t *const *f2, const uint64_t *const *f3, uint32_t flags, uint64_t *const *out);
/* f4 -- the same two initialisations with f1's non-zeros SPREAD OVER SEVERAL GPUs (worth it from dim ~ 24).
 * Every rank passes a disjoint subset of f1's (index, value) pairs -- any partition -- and all of f3 / g.  A rank's scatter is a
 * partial sum of a_hg, so the ranks' dense tables are added with ONE table-sized integer all-reduce of the widened limbs
 * (2^dim x 8 uint64 lanes, 64 bytes per entry) and folded back mod p on the device (sc_wide_reduce_table).  f1(g,.,.) stays
 * distributed: f1g_* receive the fold of THIS rank's entries (a key may occur on several ranks; its true value is the sum) and
 * are what the rank passes to sc_gkr_phase_two_sharded.
 *   comm_or_null + h_g (lanes_or_null == NULL): the library all-reduces over `comm` (RCCL or host transport; NULL or one rank =
 *       the unsharded call) and writes the finished table;
 *   lanes_or_null != NULL: no communication -- the rank's contribution is left as lanes for the CALLER's all-reduce (then
 *       sc_wide_reduce_table); h_g_or_null, if given, receives the rank's own partial table.
 * flags: SC_TABLES_ON_DEVICE as for sc_gkr_phase_one (lanes_or_null follows it too). */
SC_API int sc_gkr_phase_one_sharded(sc_comm *comm_or_null, const uint64_t *f1_idx, const uint64_t *f1_vals, uint64_t nnz_local, uint32_t dim,
                                    const uint64_t *f3, const uint64_t *g, uint32_t flags, uint64_t *h_g_or_null, uint64_t *lanes_or_null,
                                    uint64_t *f1g_idx, uint64_t *f1g_vals, uint64_t *f1g_nnz);
SC_API int sc_gkr_phase_two_sharded(sc_comm *comm_or_null, const uint64_t *f1g_idx, const uint64_t *f1g_vals, uint64_t nnz_local, uint32_t dim,
                                    const uint64_t *u, uint32_t flags, uint64_t *f1_gu_or_null, uint64_t *lanes_or_null);
/* GKRRoundSumcheck::prove (mod.rs:93-139) over several GPUs END TO END: the two initialisations as above (every rank passes its own
 * subset of f1's non-zeros, and ALL of f2, f3, g) and BOTH sumcheck phases sharded like sc_ml_prove_sharded -- rank r proves over
 * entries [r 2^dim / G, (r+1) 2^dim / G) of the phase's two tables, one all-reduce of the three evaluations per round, early gather,
 * replicated tail; f2(u) is evaluated on every rank and scales the rank's own slice of f3.  `rng` continues the caller's transcript
 * exactly as sc_gkr_prove does (no PolynomialInfo is fed: mod.rs:108-133).  out_proof: 2 x dim x 3 x 4, out_uv_or_null: 2 x dim x 4;
 * identical on every rank.  nranks a power of two below 2^dim.  Worth it from dim ~ 24 (config 5, dim = 20, belongs on one GPU). */
SC_API int sc_gkr_prove_sharded(sc_comm *comm, sc_rng *rng, const uint64_t *f1_idx, const uint64_t *f1_vals, uint64_t nnz_local, uint32_t dim,
                                const uint64_t *f2, const uint64_t *f3, const uint64_t *g, uint32_t flags, uint64_t *out_proof,
                                uint64_t *out_uv_or_null);
/* n elements of 8 summed uint64 lanes -> canonical Montgomery limbs, on the GPU (sc_wide_reduce is the host twin for a handful
 * of elements).  flags: SC_TABLES_ON_DEVICE => lanes / out are device pointers. */
SC_API int sc_wide_reduce_table(const uint64_t *lanes, uint64_t n, uint64_t *out, uint32_t flags);
/* out[i] = scalar * in[i], i < n: `DenseMultilinearExtension::zero() += (f2(u), &f3)` of start_phase2_sumcheck (mod.rs:71-75).
 * flags: SC_TABLES_ON_DEVICE => in / out are device pointers.  scalar: 4 limbs (host). */
SC_API int sc_dense_scale(const uint64_t *in, uint64_t n, const uint64_t *scalar, uint64_t *out, uint32_t flags);

/* ListOfProductsOfPolynomials::evaluate (src/ml_sumcheck/data_structures.rs:99-109): sum_k c_k prod_j T_j(point),
 * the oracle query every reference test ends with (test.rs:71-74) and GKR's f2.evaluate(u) (gkr_round_sumcheck/
 * mod.rs:122).  point: num_vars x 4 limbs, point[0] binds index bit 0.  The U table evaluations run on the device
 * (tables host or device per desc->flags, never modified); out_table_values_or_null receives them (U x 4).
 * num_vars == 0 is allowed here (a table is its single entry). */
SC_API int sc_poly_evaluate(const sc_poly_desc *desc, const uint64_t *point, uint64_t *out_value, uint64_t *out_table_values_or_null);

/* SparseMultilinearExtension::evaluate (ark-poly; the f1(g,u,v) factor of GKRRoundSumcheckSubClaim::verify_subclaim,
 * src/gkr_round_sumcheck/data_structures.rs:33-56): idx distinct, < 2^num_vars, num_vars <= 63; point: num_vars x 4. */
SC_API int sc_sparse_evaluate(const uint64_t *idx, const uint64_t *vals, uint64_t nnz, uint32_t num_vars, const uint64_t *point,
                              uint64_t *out);

/* ---- the oracle queries behind a batch of proofs ---------------------------------------------------------------------------------
 * What a caller of sc_ml_prove_batch / sc_gkr_prove_batch does next -- evaluate every instance at the point its proof ended on -- in
 * ONE call instead of n (or 3 n).  Within the envelope below the whole batch is one upload, one kernel launch (two for GKR, back to back),
 * one copy back and one synchronisation; no kernel waits for the host.  Both calls are TOTAL over shapes: beyond the envelope, with policy
 * "batch" = 0, or while a concurrent call holds the batch work areas, the instances run one after the other through sc_poly_evaluate /
 * sc_sparse_evaluate inside the call, with the same bits.  Only argument errors fail: n == 0 is SC_OK and touches nothing; everything the
 * host can check (null arrays or entries, non-canonical points / coefficients / g / uv, product indices out of range, structure
 * mismatch, dim out of range, a host-resident f1 index with a bit at or above 3 dim) is checked before any HIP call, the lowest failing
 * instance decides the status and sc_last_error() starts with "instance %u: ".  Work areas are sc_ml_prove_batch's (sc_release_caches). */
/* n x ListOfProductsOfPolynomials::evaluate (data_structures.rs:99-109), one point per instance.  descs[i]: n descriptors of ONE
 * structure (sc_ml_prove_batch's rule, check and error text); tables host or device per descs[0].flags, only read; a table pointer may
 * repeat inside an instance or across instances.  points: n x num_vars x 4 limbs, instance-major; out_values: n x 4;
 * out_table_values_or_null: n x U x 4.  num_vars == 0 is allowed.  Instance i's outputs are bit for bit what
 * sc_poly_evaluate(&descs[i], points + i * num_vars * 4, ...) returns.  One workgroup per (instance, table) up to num_vars = 14. */
SC_API int sc_poly_evaluate_batch(const sc_poly_desc *descs, uint32_t n, const uint64_t *points,
                                  uint64_t *out_values, uint64_t *out_table_values_or_null);
/* n x the three oracle queries of GKRRoundSumcheckSubClaim::verify_subclaim (data_structures.rs:33-56).  The input arrays are exactly
 * sc_gkr_prove_batch's (pointers may repeat: one f1 may serve many instances; flags: SC_TABLES_ON_DEVICE as there); uv is the
 * n x 2 x dim x 4 array sc_gkr_prove_batch writes as out_uv (host).  out_evals: n x 4 x 4 limbs -- f1(g,u,v), f2(u), f3(v) and their
 * product, which is what the caller compares with expected_evaluation.  f1 as in sc_gkr_prove_batch: repeated indices add up, any order,
 * zero values, nnz = 0 gives zero; for distinct indices f1(g,u,v) is bit for bit sc_sparse_evaluate at the point g | u | v, and f2(u),
 * f3(v) are bit for bit sc_poly_evaluate of the one-table polynomial.  1 <= dim <= 21, else SC_ERR_BAD_ARG.  One workgroup per instance for
 * dim <= 9 and nnz[i] <= 64 x 2^dim.  An out-of-range index in a device-resident list is found on the device in front of the launch
 * (SC_ERR_BAD_ARG, "instance %u: f1 has an index out of range"), never followed. */
SC_API int sc_gkr_subclaim_batch(uint32_t n, uint32_t dim,
                                 const uint64_t *const *f1_idx, const uint64_t *const *f1_vals, const uint64_t *nnz,
                                 const uint64_t *const *f2, const uint64_t *const *f3, const uint64_t *const *g,
                                 const uint64_t *uv, uint32_t flags, uint64_t *out_evals);

/* The GKR entry points keep their device scratch (about 1 GB at dim = 20) and a two-table prover handle in a process-wide
 * cache between calls (allocating and freeing them costs more than a millisecond per call), sc_poly_evaluate / sc_fix_variables keep
 * their work areas (an eighth of the tables) and stream, and sc_ml_prove keeps the last prover it built (bound-table buffers of
 * at most 16 GiB) for the next one-shot proof of the same shape; sc_ml_prove_batch keeps its message pages, mailboxes and
 * staging area.  This releases all of it. */
SC_API int sc_release_caches(void);
/* Upper bound, in bytes of device memory, of what EACH of those three caches may keep between calls (default 16 GiB; 0 = nothing is
 * kept: every call allocates and frees its own, as a library without caches would).  Lowering the limit releases what is cached now. */
SC_API int sc_set_cache_limit(uint64_t bytes);
/* process-wide counters (monotone; n <= 8 words): which path the latency-bound rounds took and what had to be repeated -- what a host
 * that runs several provers on one GPU cannot see otherwise.  out[0] persistent-tail launches; [1] times a prover found the device's
 * one tail slot taken and ran its late rounds as pipelined launches instead; [2] times the slot was taken over from an interactive
 * handle whose resident kernel had already left; [3] resident kernels started by sc_prove_round; [4] calls that found theirs gone
 * (patience expired) and took the ordinary path; [5] proofs repeated after an expired device-side wait; [6] of the launches in [0],
 * those that kept the tables resident in LDS (k_tail_slices). */
SC_API int sc_library_stats(uint64_t *out, uint32_t n);
/* Library policy: process-wide integers that select between equivalent paths (every path yields the same bits; tests and A/B runs switch
 * them).  The shipped library reads NO environment variable for any of them -- a drop-in library must not change its code path with the
 * caller's environment; it reads only SC_HOST_TRACE / SC_GKR_TRACE (stderr timings) and SC_PUBLISH_TIMEOUT_MS.  Keys (default):
 *   "pipeline" (1)           0: no kernel ever waits for the host (neither the persistent tail kernels nor pipelined launches); per handle:
 *                            SC_NO_DEVICE_POLLING / sc_prover_set_polling
 *   "resident" (1)           0: the interactive sc_prove_round never keeps a kernel on the GPU between calls (per handle: sc_prover_set_resident)
 *   "tail" (1)               0: handles built from now on run their latency-bound rounds as pipelined launches, not in a persistent kernel
 *   "tail_slices" (1)        0: the latency-bound rounds never run out of LDS (k_tail_rounds / launches instead of k_tail_slices)
 *   "vram_mailbox" (1)       0: challenges go through the host-mapped mailbox even where the host could store into device memory
 *   "wide_tree" (1)          0: handles built from now on sum products of five to twelve multiplicands node by node
 *   "rccl_direct" (1)        0: communicators initialised from now on vote against direct publication (every rank then uses the publish kernel)
 *   "shard_gather_log2" (15) 1..15: shard size (log2 entries per table in the first replicated round's region) at which a sharded proof
 *                            gathers onto every rank; must be the same on every rank
 *   "gkr_direct" (1)         0: sc_gkr_prove initialises through sort + merge (the list form) instead of the bucketed kernels
 *   "wait_spins" (2^22)      bound of a device-side wait for a challenge, in polls (tests shorten it to exercise the give-up path)
 *   "staged_init" (1)        0: sc_prover_init over HOST tables copies them whole before round 1 instead of in chunks with round 1 computed
 *                            under the copy (shapes of the merged big-round kernel from 2^18 entries per table)
 *   "batch" (1)              sc_ml_prove_batch, sc_gkr_prove_batch, sc_poly_evaluate_batch, sc_gkr_subclaim_batch, sc_batch_prover_init, sc_gkr_batch_prover_init (plans batch.gkr_rounds_one_block / batch.gkr_rounds_slices / batch.gkr_rounds_serial): 0 always the serial plan; 1 the batched kernel where the shape fits it and n is at or above
 *                            the measured crossover; 2 the batched kernel for every n that fits (tests, A/B runs)
 *   "lag_single" (2)         big rounds that a table named only by single-table products skips after round 1 (0: none .. 4): its products' messages come
 *                            from class sums of the table, and one pass binds the table with every challenge it missed before the next round
 *                            (or anything else) reads it.  The proof does not depend on the value.
 *   "batch_slices" (0)       sc_batch_prover_init, sc_gkr_batch_prover_init: 1 a shape beyond one block's LDS, up to 2^16 entries per table, runs its first rounds sliced over
 *                            several blocks per instance (plan batch.rounds_slices) instead of the serial plan; read when a handle is built; "batch" = 0
 *                            still forces the serial plan.  0 until the sliced plan has been measured.  For sc_gkr_batch_prover_init the key opens
 *                            dim 10 .. 16 [nnz <= 64 x 2^dim, at most 16 GiB of work areas and cells] to plan batch.gkr_rounds_slices: both
 *                            initialisations spread over many blocks per instance, the first rounds of each phase sliced (dim >= 11).
 *   "gkr_gates_fused" (1)    sc_gkr_gates_init_batch: 0 every gate handle built from now on is composed of three multiplication-only instances per
 *                            instance (plan batch.gkr_gates_composed) even where one block per instance would hold it (batch.gkr_gates_one_block);
 *                            read when a handle is built.
 * Unknown key or value out of range: SC_ERR_BAD_ARG. */
SC_API int sc_set_policy(const char *key, int64_t value);
SC_API int sc_get_policy(const char *key, int64_t *value);
/* Launch-plan counters (process-wide, monotone): one per path the host side can choose for a round or an initialisation -- which big-round
 * kernel, which table format, which finalize, which latency-bound form, which exchange.  sc_plan_count() plans, sc_plan_name(i) their
 * names ("big.merged.round1", "tail.slices8", "sharded.p2p", "batch.gkr_eval_layers_one_block", "batch.gkr_eval_cells", ...; NULL past the
 * end), sc_plan_stats fills out[0..n).  What the GPU test
 * suite uses to prove that every plan was reached by a test that compared with the oracle (profiles/plan_coverage.json). */
SC_API uint32_t sc_plan_count(void);
SC_API const char *sc_plan_name(uint32_t i);
SC_API int sc_plan_stats(uint64_t *out, uint32_t n);

/* ---- synthetic inputs + instrumentation (bench / tests) ------------------------------------- */
/* SplitMix64-keyed uniform field elements, generated on the device: n elements of
 * stream `stream` starting at element `first`, written to device memory d_out (n x 4 limbs). */
SC_API int sc_synth_table_device(uint64_t seed, uint64_t stream, uint64_t first, uint64_t n, uint64_t *d_out);
/* Device-side timing of the handle's last sc_prove_round: milliseconds between HIP events recorded
 * on the handle's stream around the round's kernels (excludes the D2H of the evaluations).  The events
 * are only recorded while sc_prover_set_timing(p, 1) is in effect (they cost a few microseconds per round). */
SC_API int sc_prover_last_round_ms(sc_prover *p, float *ms);
/* Per-product instrumentation: with timing on, every product kernel launch is bracketed by HIP events on the
 * handle's stream; sc_prover_get_timing returns the accumulated device milliseconds and launch counts per
 * product (K entries each) and the accumulated per-round span (all kernels of a round incl. finalize) of the rounds
 * that were launched with events: inside sc_ml_prove / sc_gkr_prove the latency-bound late rounds are pipelined
 * (enqueued before their challenge exists) and record none.
 * When a round runs as one launch over all its products (every product has <= 4 multiplicands: k_round_tree),
 * that launch is reported under product 0 and the other products report no launches. */
SC_API int sc_prover_set_timing(sc_prover *p, int on);
SC_API int sc_prover_get_timing(sc_prover *p, double *ms_per_product, uint64_t *launches_per_product, double *rounds_ms);
/* the same per ROUND (num_vars entries, index = round - 1): device time of that round's big-round kernel launch(es) and how many timed
 * proofs contributed; zero for the latency-bound rounds, which record no events.  bench.py's roofline.per_round. */
SC_API int sc_prover_get_round_timing(sc_prover *p, double *ms_per_round, uint64_t *launches_per_round);
/* Rewind a handle to round 0 without reallocating (repeated proofs over resident tables).  Borrowing handle:
 * tables_or_null = new device pointers, or NULL for the same tables.  Copying handle: tables are required and
 * copied in again (device pointers iff flags has SC_TABLES_ON_DEVICE). */
SC_API int sc_prover_reset(sc_prover *p, const uint64_t *const *tables_or_null, uint32_t flags);
/* Host logic of the claim identity, exposed for tests: out[s], s = 0..M, are the weights of a degree-M polynomial's
 * values at the kernel nodes 0, 1, inf (= leading coefficient), -1, 2 in its value at the point r, i.e.
 * f(r) = sum_s out[s] * f(node_s).  1 <= M <= 4; r canonical Montgomery limbs; no device needed. */
SC_API int sc_claim_weights(uint32_t M, const uint64_t *r, uint64_t *out);
/* Elementwise field arithmetic on host arrays of n elements, computed on the GPU (arithmetic parity tests):
 * op 0 mul (production path) | 1 add | 2 sub | 3 mul, plain-C++ CIOS | 4 mul, Comba asm | 5 a[i] * b[0] with b[0] uniform. */
SC_API int sc_fr_elementwise(int op, const uint64_t *a, const uint64_t *b, uint64_t *out, uint64_t n);
/* Elementwise micro-kernel: dependent chains of `reps` field ops per lane, 4 chains per lane (ceilings):
 * variant 0 mul CIOS | 1 add | 2 mul Comba | 3 mul Comba by a uniform operand | 4 two Comba products interleaved. */
SC_API int sc_bench_modmul(uint64_t n_threads, uint32_t reps, uint32_t variant, float *ms_out, uint64_t *checksum_out);

#ifdef __cplusplus
}
#endif
#endif /* SUMCHECK_HIP_H */
