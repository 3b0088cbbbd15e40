//! `extern "C"` binding of `libsumcheck_hip.so` (C ABI: `include/sumcheck_hip.h`, SC_ABI_VERSION 5) exposed with the
//! signatures of the reference's public API:
//!
//! | here | reference |
//! |---|---|
//! | [`prover_init`], [`prove_round`]            | `IPForMLSumcheck::{prover_init, prove_round}` `src/ml_sumcheck/protocol/prover.rs:49,74` |
//! | [`prove`], [`prove_as_subprotocol`]         | `MLSumcheck::{prove, prove_as_subprotocol}` `src/ml_sumcheck/mod.rs:42,50` |
//! | [`gkr_prover_init_batch`], [`gkr_prove_round_batch`], [`gkr_finish_batch`] | (new) the rounds of many small `GKRRoundSumcheck::prove` under the caller's transcript (`rng: &mut impl FeedableRNG`), one call per round |
//! | [`gkr_next_layer_batch`] | (new) the same handle onto the next layer's `f2`, `f3`, `g` (and `f1`) without a rebuild: one handle for the layers of a GKR prover |
//! | [`gkr_prover_init_batch_two_point`], [`gkr_next_layer_batch_two_point`] | (new) the same handle in two-point form: `alpha eq(g, .) + beta eq(g2, .)` where `eq(g, .)` stands, for the layers of a GKR prover below the output layer |
//! | [`prover_init_batch`], [`prove_round_batch`] | (new) `states.par_iter_mut().zip(msgs).map(prove_round)`: one round of many small provers in one call, the caller's transcript |
//! | [`prove_batch`]                            | (new) `polys.par_iter().map(MLSumcheck::prove)`: many small instances of one structure in one call |
//! | [`evaluate`]                                | `ListOfProductsOfPolynomials::evaluate` `src/ml_sumcheck/data_structures.rs:99` |
//! | [`initialize_phase_one`], [`initialize_phase_two`] | `src/gkr_round_sumcheck/mod.rs:22,57` |
//! | [`gkr_prove`]                               | `GKRRoundSumcheck::prove` `src/gkr_round_sumcheck/mod.rs:93` |
//! | [`prove_sharded`]                           | (new) one rank of a multi-GPU `MLSumcheck::prove_as_subprotocol` |
//!
//! The reference crate is `#![forbid(unsafe_code)]` (`src/lib.rs:1`), so the FFI lives in this separate crate.
//! An `Fr` is passed as the address of its 4 x u64 Montgomery limbs: `Fp<MontBackend<FrConfig,4>,4>` is a transparent
//! wrapper of `BigInt<4>([u64; 4])`, which is exactly the C ABI's element layout.
//!
//! `ProverMsg::evaluations` and `GKRProof`'s fields are `pub(crate)` in the reference (`prover.rs:16`,
//! `gkr_round_sumcheck/data_structures.rs:10-11`).  A `ProverMsg` is therefore built here through its derived
//! `CanonicalDeserialize` (a `Vec<F>`: u64 length + elements) -- which keeps `MLSumcheck::verify` and
//! `GKRRoundSumcheck::verify` usable on the result unchanged; a `GKRProof` cannot be built outside the reference crate at all,
//! so [`gkr_prove`] returns the two message lists ([`HipGKRProof`]) and the one-line constructor a maintainer would add
//! to the reference (`GKRProof { phase1_sumcheck_msgs, phase2_sumcheck_msgs }`) is shown in INTEGRATION.md.
//!
//! NOT BUILT in the image this repository was developed in (no cargo); kept in sync with the header by hand.
#![allow(non_camel_case_types)]
use ark_ff::{BigInt, Fp, MontBackend, MontConfig, PrimeField};
use ark_poly::{DenseMultilinearExtension, SparseMultilinearExtension};
use ark_serialize::{CanonicalDeserialize, CanonicalSerialize};
use ark_std::os::raw::{c_char, c_int, c_void};
use ark_std::rc::Rc;
use ark_sumcheck::ml_sumcheck::data_structures::ListOfProductsOfPolynomials;
use ark_sumcheck::ml_sumcheck::protocol::prover::{ProverMsg, ProverState};
use ark_sumcheck::ml_sumcheck::protocol::verifier::VerifierMsg;
use ark_sumcheck::ml_sumcheck::protocol::IPForMLSumcheck;
use ark_sumcheck::ml_sumcheck::Proof;
use ark_sumcheck::rng::FeedableRNG;

#[repr(C)]
pub struct sc_poly_desc {
    pub num_vars: u32,
    pub max_multiplicands: u32,
    pub n_products: u32,
    pub coeffs: *const u64,
    pub prod_offsets: *const u32,
    pub prod_indices: *const u32,
    pub n_tables: u32,
    pub tables: *const *const u64,
    pub flags: u32,
}
#[repr(C)]
pub struct sc_prover {
    _private: [u8; 0],
}
#[repr(C)]
pub struct sc_rng {
    _private: [u8; 0],
}
#[repr(C)]
pub struct sc_comm {
    _private: [u8; 0],
}
#[repr(C)]
pub struct sc_batch_prover {
    _private: [u8; 0],
}
#[repr(C)]
pub struct sc_gkr_batch_prover {
    _private: [u8; 0],
}

pub const SC_ABI_VERSION: c_int = 5;
pub const SC_OK: c_int = 0;
pub const SC_ERR_CONSTANT_POLY: c_int = 1;
pub const SC_ERR_FIRST_ROUND_HAS_MSG: c_int = 2;
pub const SC_ERR_MISSING_MSG: c_int = 3;
pub const SC_ERR_NOT_ACTIVE: c_int = 4;
pub const SC_ERR_BAD_ARG: c_int = 5;
pub const SC_TABLES_ON_DEVICE: u32 = 1;
pub const SC_TABLES_BORROW: u32 = 2;
pub const SC_NO_DEVICE_POLLING: u32 = 8; // a host with HIP streams of its own: no kernel of this handle ever waits for the host

pub type sc_allreduce_u64_fn = Option<unsafe extern "C" fn(ctx: *mut c_void, inout: *mut u64, count: usize) -> c_int>;
pub type sc_allgather_fn = Option<unsafe extern "C" fn(ctx: *mut c_void, send: *const c_void, recv: *mut c_void, bytes: usize) -> c_int>;

extern "C" {
    pub fn sc_abi_version() -> c_int;
    pub fn sc_last_error() -> *const c_char;
    pub fn sc_set_device(ordinal: c_int) -> c_int;
    pub fn sc_prover_init(desc: *const sc_poly_desc, out: *mut *mut sc_prover) -> c_int;
    pub fn sc_prover_init_streamed(desc: *const sc_poly_desc, chunk_log2: u32, out: *mut *mut sc_prover) -> c_int;
    pub fn sc_prove_round(p: *mut sc_prover, r_or_null: *const u64, out_evals: *mut u64) -> c_int;
    pub fn sc_prover_push_randomness(p: *mut sc_prover, r: *const u64) -> c_int;
    pub fn sc_prover_state(p: *mut sc_prover, randomness: *mut u64, n_randomness: *mut u32, tables_out: *mut u64, round: *mut u32) -> c_int;
    pub fn sc_prover_free(p: *mut sc_prover);
    pub fn sc_release_caches() -> c_int;
    pub fn sc_set_cache_limit(bytes: u64) -> c_int;
    pub fn sc_library_stats(out: *mut u64, n: u32) -> c_int;
    pub fn sc_set_policy(key: *const c_char, value: i64) -> c_int;
    pub fn sc_get_policy(key: *const c_char, value: *mut i64) -> c_int;
    pub fn sc_plan_count() -> u32;
    pub fn sc_plan_name(i: u32) -> *const c_char;
    pub fn sc_plan_stats(out: *mut u64, n: u32) -> c_int;
    pub fn sc_prover_set_polling(p: *mut sc_prover, allow: c_int) -> c_int;
    pub fn sc_prover_set_resident(p: *mut sc_prover, patience_polls: u32) -> c_int;
    pub fn sc_fix_variables(input: *const u64, nv: u32, point: *const u64, k: u32, out: *mut u64, flags: u32) -> c_int;
    pub fn sc_poly_evaluate(desc: *const sc_poly_desc, point: *const u64, out_value: *mut u64, out_table_values_or_null: *mut u64) -> c_int;
    pub fn sc_poly_evaluate_batch(descs: *const sc_poly_desc, n: u32, points: *const u64, out_values: *mut u64, out_table_values_or_null: *mut u64) -> c_int;
    pub fn sc_gkr_subclaim_batch(n: u32, dim: u32, f1_idx: *const *const u64, f1_vals: *const *const u64, nnz: *const u64, f2: *const *const u64,
                                 f3: *const *const u64, g: *const *const u64, uv: *const u64, flags: u32, out_evals: *mut u64) -> c_int;
    pub fn sc_sparse_evaluate(idx: *const u64, vals: *const u64, nnz: u64, num_vars: u32, point: *const u64, out: *mut u64) -> c_int;
    pub fn sc_ml_prove(desc: *const sc_poly_desc, rng_or_null: *mut sc_rng, out_proof: *mut u64, out_state_or_null: *mut *mut sc_prover) -> c_int;
    pub fn sc_ml_prove_batch(descs: *const sc_poly_desc, n: u32, rngs_or_null: *const *mut sc_rng, out_proofs: *mut u64,
                             out_randomness_or_null: *mut u64) -> c_int;
    pub fn sc_ml_verify(num_vars: u32, max_multiplicands: u32, claimed_sum: *const u64, proof: *const u64, proof_elems: u64,
                        rng_or_null: *mut sc_rng, out_point: *mut u64, out_expected: *mut u64) -> c_int;
    pub fn sc_gkr_phase_one(f1_idx: *const u64, f1_vals: *const u64, nnz: u64, dim: u32, f3: *const u64, g: *const u64, flags: u32,
                            h_g: *mut u64, f1g_idx: *mut u64, f1g_vals: *mut u64, f1g_nnz: *mut u64) -> c_int;
    pub fn sc_gkr_phase_two(f1g_idx: *const u64, f1g_vals: *const u64, nnz: u64, dim: u32, u: *const u64, flags: u32, f1_gu: *mut u64) -> c_int;
    pub fn sc_gkr_prove(rng: *mut sc_rng, f1_idx: *const u64, f1_vals: *const u64, nnz: u64, dim: u32, f2: *const u64, f3: *const u64,
                        g: *const u64, flags: u32, out_proof: *mut u64, out_uv_or_null: *mut u64) -> c_int;
    pub fn sc_gkr_prove_batch(n: u32, dim: u32, rngs: *const *mut sc_rng, f1_idx: *const *const u64, f1_vals: *const *const u64, nnz: *const u64,
                              f2: *const *const u64, f3: *const *const u64, g: *const *const u64, flags: u32, out_proofs: *mut u64,
                              out_uv_or_null: *mut u64) -> c_int;
    pub fn sc_gkr_prove_sharded(comm: *mut sc_comm, rng: *mut sc_rng, f1_idx: *const u64, f1_vals: *const u64, nnz_local: u64, dim: u32, f2: *const u64,
                                f3: *const u64, g: *const u64, flags: u32, out_proof: *mut u64, out_uv_or_null: *mut u64) -> c_int;
    pub fn sc_comm_unique_id(out128: *mut u8) -> c_int;
    pub fn sc_comm_init(id128: *const u8, rank: c_int, nranks: c_int, out: *mut *mut sc_comm) -> c_int;
    pub fn sc_comm_init_host(rank: c_int, nranks: c_int, allreduce: sc_allreduce_u64_fn, allgather: sc_allgather_fn, ctx: *mut c_void,
                             out: *mut *mut sc_comm) -> c_int;
    pub fn sc_comm_init_p2p(group_id: u64, rank: c_int, nranks: c_int, out: *mut *mut sc_comm) -> c_int;
    pub fn sc_comm_free(comm: *mut sc_comm);
    pub fn sc_comm_info(comm: *mut sc_comm, rank_out: *mut c_int, nranks_out: *mut c_int, kind_out: *mut c_int) -> c_int;
    pub fn sc_comm_exchange_bench(comm: *mut sc_comm, n_words: u32, iters: u32, us_mean_out: *mut f64, us_min_out_or_null: *mut f64) -> c_int;
    pub fn sc_set_publish_timeout_ms(ms: u32) -> c_int;
    pub fn sc_ml_prove_sharded(p: *mut sc_prover, comm: *mut sc_comm, rng_or_null: *mut sc_rng, nv_total: u32, out_proof: *mut u64,
                               out_randomness: *mut u64) -> c_int;
    pub fn sc_rng_setup() -> *mut sc_rng;
    pub fn sc_rng_free(rng: *mut sc_rng);
    pub fn sc_rng_feed_bytes(rng: *mut sc_rng, buf: *const u8, len: usize);
}

/// Field types whose in-memory form is 4 x u64 Montgomery limbs (BLS12-381 Fr and friends).
pub trait Limbs4: PrimeField {
    fn limbs(&self) -> *const u64;
    fn from_limbs(l: [u64; 4]) -> Self;
    fn to_limbs(&self) -> [u64; 4] {
        unsafe { *(self.limbs() as *const [u64; 4]) }
    }
}
impl<P: MontConfig<4>> Limbs4 for Fp<MontBackend<P, 4>, 4> {
    fn limbs(&self) -> *const u64 {
        self.0 .0.as_ptr()
    }
    fn from_limbs(l: [u64; 4]) -> Self {
        Fp(BigInt(l), core::marker::PhantomData) // raw Montgomery limbs, no conversion
    }
}

fn panic_like_reference(code: c_int) -> ! {
    // the same messages as the reference's panic!s (prover.rs:51,80,91,97)
    match code {
        SC_ERR_CONSTANT_POLY => panic!("Attempt to prove a constant."),
        SC_ERR_FIRST_ROUND_HAS_MSG => panic!("first round should be prover first."),
        SC_ERR_MISSING_MSG => panic!("verifier message is empty"),
        SC_ERR_NOT_ACTIVE => panic!("Prover is not active"),
        _ => {
            let msg = unsafe { std::ffi::CStr::from_ptr(sc_last_error()) }.to_string_lossy().into_owned();
            panic!("libsumcheck_hip: status {code}: {msg}")
        },
    }
}
fn check(rc: c_int) {
    if rc != SC_OK {
        panic_like_reference(rc)
    }
}

/// `ProverMsg { evaluations }` from the library's limbs.  The field is `pub(crate)` in the reference, so the message is
/// rebuilt through its derived `CanonicalDeserialize`: a `Vec<F>` is a u64-LE length followed by the elements.
fn prover_msg<F: Limbs4>(evals: &[[u64; 4]]) -> ProverMsg<F> {
    let v: Vec<F> = evals.iter().map(|l| F::from_limbs(*l)).collect();
    let mut bytes = Vec::new();
    v.serialize_uncompressed(&mut bytes).expect("serialising to a Vec cannot fail");
    ProverMsg::<F>::deserialize_uncompressed_unchecked(&bytes[..]).expect("a serialised Vec<F> is a ProverMsg")
}

struct Flattened {
    coeffs: Vec<[u64; 4]>,
    offsets: Vec<u32>,
    indices: Vec<u32>,
    tables: Vec<*const u64>,
}
impl Flattened {
    fn desc(&self, num_vars: usize, max_multiplicands: usize, flags: u32) -> sc_poly_desc {
        sc_poly_desc {
            num_vars: num_vars as u32,
            max_multiplicands: max_multiplicands as u32,
            n_products: self.coeffs.len() as u32,
            coeffs: self.coeffs.as_ptr() as *const u64,
            prod_offsets: self.offsets.as_ptr(),
            prod_indices: self.indices.as_ptr(),
            n_tables: self.tables.len() as u32,
            tables: self.tables.as_ptr(),
            flags,
        }
    }
}
fn flatten<F: Limbs4>(polynomial: &ListOfProductsOfPolynomials<F>) -> Flattened {
    let coeffs = polynomial.products.iter().map(|(c, _)| c.to_limbs()).collect();
    let mut offsets = vec![0u32];
    let mut indices = Vec::new();
    for (_, idx) in &polynomial.products {
        indices.extend(idx.iter().map(|&i| i as u32));
        offsets.push(indices.len() as u32);
    }
    let tables = polynomial.flattened_ml_extensions.iter().map(|m: &Rc<DenseMultilinearExtension<F>>| m.evaluations.as_ptr() as *const u64).collect();
    Flattened { coeffs, offsets, indices, tables }
}

/// `ProverState` (reference `prover.rs:19-33`) with its tables resident in HBM.  [`HipProverState::to_prover_state`] copies the
/// state back into the reference's own struct (all of whose fields are `pub`).
pub struct HipProverState<F: Limbs4> {
    handle: *mut sc_prover,
    pub list_of_products: Vec<(F, Vec<usize>)>,
    pub n_tables: usize,
    pub num_vars: usize,
    pub max_multiplicands: usize,
}
impl<F: Limbs4> Drop for HipProverState<F> {
    fn drop(&mut self) {
        unsafe { sc_prover_free(self.handle) }
    }
}
impl<F: Limbs4> HipProverState<F> {
    pub fn round(&self) -> usize {
        let mut r = 0u32;
        check(unsafe { sc_prover_state(self.handle, core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut(), &mut r) });
        r as usize
    }
    /// A host that runs HIP work of its own on the device: `false` = no kernel of this handle ever waits for the host (every round is
    /// launched after its challenge is known); see the interference contract in `sumcheck_hip.h`.
    pub fn set_polling(&mut self, allow: bool) {
        check(unsafe { sc_prover_set_polling(self.handle, allow as c_int) });
    }
    /// Patience (in ~2 us polls; 0 = off) of the kernel that serves the late rounds of `prove_round` called round by round.
    pub fn set_resident(&mut self, patience_polls: u32) {
        check(unsafe { sc_prover_set_resident(self.handle, patience_polls) });
    }
    /// the reference's `ProverState`: randomness, product list, the (partially bound) tables, round
    pub fn to_prover_state(&self) -> ProverState<F> {
        let round = self.round();
        let bound = round.saturating_sub(1);
        let n = 1usize << (self.num_vars - bound);
        let mut rand = vec![[0u64; 4]; self.num_vars + 1];
        let mut n_rand = 0u32;
        let mut tabs = vec![[0u64; 4]; self.n_tables * n];
        check(unsafe { sc_prover_state(self.handle, rand.as_mut_ptr() as *mut u64, &mut n_rand, tabs.as_mut_ptr() as *mut u64, core::ptr::null_mut()) });
        ProverState {
            randomness: rand[..n_rand as usize].iter().map(|l| F::from_limbs(*l)).collect(),
            list_of_products: self.list_of_products.clone(),
            flattened_ml_extensions: tabs
                .chunks(n)
                .map(|t| DenseMultilinearExtension::from_evaluations_vec(self.num_vars - bound, t.iter().map(|l| F::from_limbs(*l)).collect()))
                .collect(),
            num_vars: self.num_vars,
            max_multiplicands: self.max_multiplicands,
            round,
        }
    }
}

/// `IPForMLSumcheck::prover_init` (reference `prover.rs:49-69`): flattens the product list and uploads every unique table once.
pub fn prover_init<F: Limbs4>(polynomial: &ListOfProductsOfPolynomials<F>) -> HipProverState<F> {
    let flat = flatten(polynomial);
    let desc = flat.desc(polynomial.num_variables, polynomial.max_multiplicands, 0);
    let mut handle = core::ptr::null_mut();
    check(unsafe { sc_prover_init(&desc, &mut handle) });
    HipProverState {
        handle,
        list_of_products: polynomial.products.clone(),
        n_tables: polynomial.flattened_ml_extensions.len(),
        num_vars: polynomial.num_variables,
        max_multiplicands: polynomial.max_multiplicands,
    }
}

/// Out-of-core `prover_init` (`sc_prover_init_streamed`): the tables of `polynomial` are NOT copied to HBM as a whole; rounds 1 and 2 stream
/// them from host memory in chunks of `2^chunk_log2` entries (0 = default).  The borrow of `polynomial` makes the compiler hold the
/// tables alive and unchanged for as long as the state exists, which covers the two rounds that read them.
pub fn prover_init_streamed<'a, F: Limbs4>(polynomial: &'a ListOfProductsOfPolynomials<F>, chunk_log2: u32) -> (HipProverState<F>, core::marker::PhantomData<&'a ()>) {
    let flat = flatten(polynomial);
    let desc = flat.desc(polynomial.num_variables, polynomial.max_multiplicands, 0);
    let mut handle = core::ptr::null_mut();
    check(unsafe { sc_prover_init_streamed(&desc, chunk_log2, &mut handle) });
    (
        HipProverState {
            handle,
            list_of_products: polynomial.products.clone(),
            n_tables: polynomial.flattened_ml_extensions.len(),
            num_vars: polynomial.num_variables,
            max_multiplicands: polynomial.max_multiplicands,
        },
        core::marker::PhantomData,
    )
}

/// `IPForMLSumcheck::prove_round` (reference `prover.rs:74-153`), same signature: `&Option<VerifierMsg<F>>` in, `ProverMsg<F>` out.
pub fn prove_round<F: Limbs4>(prover_state: &mut HipProverState<F>, v_msg: &Option<VerifierMsg<F>>) -> ProverMsg<F> {
    let mut out = vec![[0u64; 4]; prover_state.max_multiplicands + 1];
    let r = v_msg.as_ref().map_or(core::ptr::null(), |m| m.randomness.limbs());
    check(unsafe { sc_prove_round(prover_state.handle, r, out.as_mut_ptr() as *mut u64) });
    prover_msg(&out)
}

/// `MLSumcheck::prove_as_subprotocol` (reference `src/ml_sumcheck/mod.rs:50-70`) over the CALLER's transcript: any
/// `FeedableRNG`, fed and sampled here exactly as the reference does, one `sc_prove_round` per round.
pub fn prove_as_subprotocol<F: Limbs4, R: FeedableRNG>(fs_rng: &mut R, polynomial: &ListOfProductsOfPolynomials<F>) -> Result<(Proof<F>, ProverState<F>), R::Error> {
    fs_rng.feed(&polynomial.info())?; // mod.rs:54
    let mut prover_state = prover_init(polynomial);
    let mut verifier_msg = None;
    let mut prover_msgs = Vec::with_capacity(polynomial.num_variables);
    for _ in 0..polynomial.num_variables {
        let prover_msg = prove_round(&mut prover_state, &verifier_msg); // mod.rs:60
        fs_rng.feed(&prover_msg)?;
        prover_msgs.push(prover_msg);
        verifier_msg = Some(IPForMLSumcheck::sample_round(fs_rng)); // mod.rs:63
    }
    let last = verifier_msg.expect("num_variables > 0 (prover_init panics on a constant)").randomness;
    check(unsafe { sc_prover_push_randomness(prover_state.handle, last.limbs()) }); // mod.rs:65-67
    Ok((prover_msgs, prover_state.to_prover_state()))
}

/// `MLSumcheck::prove` (reference `src/ml_sumcheck/mod.rs:42-45`): the whole Fiat-Shamir loop in ONE FFI call (`sc_ml_prove`
/// with a fresh `Blake2b512Rng::setup()` transcript inside the library; the latency-bound rounds run in its persistent kernel).
pub fn prove<F: Limbs4>(polynomial: &ListOfProductsOfPolynomials<F>) -> Proof<F> {
    let flat = flatten(polynomial);
    let desc = flat.desc(polynomial.num_variables, polynomial.max_multiplicands, 0);
    let d = polynomial.max_multiplicands + 1;
    let mut proof = vec![[0u64; 4]; polynomial.num_variables.max(1) * d];
    check(unsafe { sc_ml_prove(&desc, core::ptr::null_mut(), proof.as_mut_ptr() as *mut u64, core::ptr::null_mut()) });
    proof.chunks(d).take(polynomial.num_variables).map(prover_msg).collect()
}

/// `polys.par_iter().map(MLSumcheck::prove).collect()` for instances of ONE structure (the same number of variables and the same
/// product lists; tables and coefficients are each instance's own) in one FFI call (`sc_ml_prove_batch`).  Small instances -- every
/// table of an instance within one workgroup's LDS -- are proved concurrently, a workgroup each, inside one kernel; other shapes are
/// proved one after the other inside the call.  Every proof is bit for bit what [`prove`] returns for that polynomial.  Panics like
/// [`prove`] on an invalid instance, and if the structures differ.
pub fn prove_batch<F: Limbs4>(polynomials: &[ListOfProductsOfPolynomials<F>]) -> Vec<Proof<F>> {
    if polynomials.is_empty() {
        return Vec::new();
    }
    let flats: Vec<Flattened> = polynomials.iter().map(flatten).collect();
    let descs: Vec<sc_poly_desc> = flats.iter().zip(polynomials).map(|(f, p)| f.desc(p.num_variables, p.max_multiplicands, 0)).collect();
    let (nv, d) = (polynomials[0].num_variables, polynomials[0].max_multiplicands + 1);
    let mut proofs = vec![[0u64; 4]; polynomials.len() * nv.max(1) * d];
    check(unsafe { sc_ml_prove_batch(descs.as_ptr(), descs.len() as u32, core::ptr::null(), proofs.as_mut_ptr() as *mut u64, core::ptr::null_mut()) });
    proofs.chunks(nv.max(1) * d).map(|one| one.chunks(d).take(nv).map(prover_msg).collect()).collect()
}

// The batched interactive rounds (`sc_batch_prover_*`): private declarations behind the safe wrappers below.
extern "C" {
    fn sc_batch_prover_init(descs: *const sc_poly_desc, n: u32, out: *mut *mut sc_batch_prover) -> c_int;
    fn sc_batch_prove_round(bp: *mut sc_batch_prover, r_or_null: *const u64, r_shared: u32, out_evals: *mut u64) -> c_int;
    fn sc_batch_prover_push_randomness(bp: *mut sc_batch_prover, r: *const u64, r_shared: u32) -> c_int;
    fn sc_batch_prover_state(bp: *mut sc_batch_prover, instance: u32, randomness: *mut u64, n_randomness: *mut u32, tables_out: *mut u64,
                             round: *mut u32) -> c_int;
    fn sc_batch_prover_bind_final(bp: *mut sc_batch_prover, r: *const u64, r_shared: u32, out_table_values: *mut u64) -> c_int;
    fn sc_batch_prover_reset(bp: *mut sc_batch_prover, descs_or_null: *const sc_poly_desc) -> c_int;
    fn sc_batch_prover_free(bp: *mut sc_batch_prover);
}

/// n x `ProverState` of ONE structure behind one `sc_batch_prover` handle ([`prover_init_batch`]).
pub struct HipBatchProverState<F: Limbs4> {
    handle: *mut sc_batch_prover,
    pub n: usize,
    pub num_vars: usize,
    pub max_multiplicands: usize,
    n_tables: usize,
    _f: core::marker::PhantomData<F>,
}
impl<F: Limbs4> Drop for HipBatchProverState<F> {
    fn drop(&mut self) {
        unsafe { sc_batch_prover_free(self.handle) }
    }
}
impl<F: Limbs4> HipBatchProverState<F> {
    pub fn round(&self) -> usize {
        let mut r = 0u32;
        check(unsafe { sc_batch_prover_state(self.handle, 0, core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut(), &mut r) });
        r as usize
    }
    /// the challenges instance `i` has received so far
    pub fn randomness(&self, i: usize) -> Vec<F> {
        let mut rand = vec![[0u64; 4]; self.num_vars + 1];
        let mut n_rand = 0u32;
        check(unsafe { sc_batch_prover_state(self.handle, i as u32, rand.as_mut_ptr() as *mut u64, &mut n_rand, core::ptr::null_mut(), core::ptr::null_mut()) });
        rand[..n_rand as usize].iter().map(|l| F::from_limbs(*l)).collect()
    }
    /// `prove_as_subprotocol`'s final push without a bind (`mod.rs:65-67`): one challenge per instance
    pub fn push_randomness(&mut self, v_msgs: &[VerifierMsg<F>]) {
        assert_eq!(v_msgs.len(), self.n, "one VerifierMsg per instance");
        let r: Vec<[u64; 4]> = v_msgs.iter().map(|m| m.randomness.to_limbs()).collect();
        check(unsafe { sc_batch_prover_push_randomness(self.handle, r.as_ptr() as *const u64, 0) });
    }
    /// bind the last variable after the last round: per instance the table evaluations at its point; exhausts the handle until [`Self::reset`]
    pub fn bind_final(&mut self, v_msgs: &[VerifierMsg<F>]) -> Vec<Vec<F>> {
        assert_eq!(v_msgs.len(), self.n, "one VerifierMsg per instance");
        let r: Vec<[u64; 4]> = v_msgs.iter().map(|m| m.randomness.to_limbs()).collect();
        let mut out = vec![[0u64; 4]; self.n * self.n_tables.max(1)];
        check(unsafe { sc_batch_prover_bind_final(self.handle, r.as_ptr() as *const u64, 0, out.as_mut_ptr() as *mut u64) });
        out.chunks(self.n_tables.max(1)).map(|t| t.iter().take(self.n_tables).map(|l| F::from_limbs(*l)).collect()).collect()
    }
    /// rewind to round 0 over the tables the handle holds (no allocation, no copy)
    pub fn reset(&mut self) {
        check(unsafe { sc_batch_prover_reset(self.handle, core::ptr::null()) });
    }
}

/// n x `IPForMLSumcheck::prover_init` for polynomials of ONE structure behind one handle (`sc_batch_prover_init`); the tables are copied.
/// Shapes beyond one block's LDS run n ordinary provers inside the handle (plan `batch.rounds_serial`) unless the library policy
/// `batch_slices` is 1 when the handle is built (`sc_set_policy`; default 0): then, for 1 <= num_vars <= 16, products of at most eight
/// multiplicands and a work area (96 bytes x n x tables x 2^num_vars) of at most 16 GiB, the rounds whose tables do not fit one block give
/// every instance to several blocks (plan `batch.rounds_slices`: two launches a round) and the later rounds run as within the envelope,
/// with the same bits.
pub fn prover_init_batch<F: Limbs4>(polynomials: &[ListOfProductsOfPolynomials<F>]) -> HipBatchProverState<F> {
    assert!(!polynomials.is_empty(), "a batch handle holds at least one instance");
    let flats: Vec<Flattened> = polynomials.iter().map(flatten).collect();
    let descs: Vec<sc_poly_desc> = flats.iter().zip(polynomials).map(|(f, p)| f.desc(p.num_variables, p.max_multiplicands, 0)).collect();
    let mut handle = core::ptr::null_mut();
    check(unsafe { sc_batch_prover_init(descs.as_ptr(), descs.len() as u32, &mut handle) });
    HipBatchProverState {
        handle,
        n: polynomials.len(),
        num_vars: polynomials[0].num_variables,
        max_multiplicands: polynomials[0].max_multiplicands,
        n_tables: polynomials[0].flattened_ml_extensions.len(),
        _f: core::marker::PhantomData,
    }
}

/// `states.iter_mut().zip(v_msgs).map(|(s, m)| IPForMLSumcheck::prove_round(s, m))` in one FFI call (`sc_batch_prove_round`): `None` on
/// the first call, then one `VerifierMsg` per instance -- from whatever transcript(s) the caller keeps.  Message i is bit for bit
/// [`prove_round`]'s for instance i.
pub fn prove_round_batch<F: Limbs4>(state: &mut HipBatchProverState<F>, v_msgs: Option<&[VerifierMsg<F>]>) -> Vec<ProverMsg<F>> {
    let d = state.max_multiplicands + 1;
    let mut out = vec![[0u64; 4]; state.n * d];
    match v_msgs {
        None => check(unsafe { sc_batch_prove_round(state.handle, core::ptr::null(), 0, out.as_mut_ptr() as *mut u64) }),
        Some(ms) => {
            assert_eq!(ms.len(), state.n, "one VerifierMsg per instance");
            let r: Vec<[u64; 4]> = ms.iter().map(|m| m.randomness.to_limbs()).collect();
            check(unsafe { sc_batch_prove_round(state.handle, r.as_ptr() as *const u64, 0, out.as_mut_ptr() as *mut u64) })
        }
    }
    out.chunks(d).map(prover_msg).collect()
}

/// The library keeps device memory between calls so that one-shot use costs what a kept prover costs: the last prover it built (up to
/// 16 GiB of bound-table buffers), the work areas of `evaluate` / `fix_variables`, the GKR scratch.  This gives all of it back.
pub fn release_caches() {
    check(unsafe { sc_release_caches() });
}
/// Upper bound (bytes of device memory) of what each of those caches may keep between calls; 0 = nothing is kept.
pub fn set_cache_limit(bytes: u64) {
    check(unsafe { sc_set_cache_limit(bytes) });
}

/// `ListOfProductsOfPolynomials::evaluate` (reference `src/ml_sumcheck/data_structures.rs:99-109`): the oracle query that
/// follows a proof, with every table folded on the GPU (`sc_poly_evaluate`).
pub fn evaluate<F: Limbs4>(polynomial: &ListOfProductsOfPolynomials<F>, point: &[F]) -> F {
    assert_eq!(point.len(), polynomial.num_variables, "wrong number of variables");
    let flat = flatten(polynomial);
    let desc = flat.desc(polynomial.num_variables, polynomial.max_multiplicands, 0);
    let pt: Vec<[u64; 4]> = point.iter().map(|x| x.to_limbs()).collect();
    let mut out = [0u64; 4];
    check(unsafe { sc_poly_evaluate(&desc, pt.as_ptr() as *const u64, out.as_mut_ptr(), core::ptr::null_mut()) });
    F::from_limbs(out)
}

/// `polys.iter().zip(points).map(|(p, x)| p.evaluate(x))` for polynomials of ONE structure in one FFI call (`sc_poly_evaluate_batch`):
/// what follows [`prove_batch`] -- one more call, not n.  `points[i]` is the point polynomial i's proof ended on.  Every value is bit for
/// bit what [`evaluate`] returns for that polynomial and point.
pub fn evaluate_batch<F: Limbs4>(polynomials: &[ListOfProductsOfPolynomials<F>], points: &[Vec<F>]) -> Vec<F> {
    assert_eq!(polynomials.len(), points.len(), "one point per polynomial");
    if polynomials.is_empty() {
        return Vec::new();
    }
    let nv = polynomials[0].num_variables;
    let flats: Vec<Flattened> = polynomials.iter().map(flatten).collect();
    let descs: Vec<sc_poly_desc> = flats.iter().zip(polynomials).map(|(f, p)| f.desc(p.num_variables, p.max_multiplicands, 0)).collect();
    let mut pts: Vec<[u64; 4]> = Vec::with_capacity(points.len() * nv);
    for x in points {
        assert_eq!(x.len(), nv, "wrong number of variables");
        pts.extend(x.iter().map(|e| e.to_limbs()));
    }
    let mut out = vec![[0u64; 4]; polynomials.len()];
    check(unsafe { sc_poly_evaluate_batch(descs.as_ptr(), descs.len() as u32, pts.as_ptr() as *const u64, out.as_mut_ptr() as *mut u64, core::ptr::null_mut()) });
    out.into_iter().map(F::from_limbs).collect()
}

// ---- GKR round sumcheck (reference src/gkr_round_sumcheck/mod.rs) ------------------------------------------------------------
/// `SparseMultilinearExtension.evaluations` (a map index -> value) as the two parallel arrays the C ABI takes
fn sparse_arrays<F: Limbs4>(f: &SparseMultilinearExtension<F>) -> (Vec<u64>, Vec<[u64; 4]>) {
    let mut idx = Vec::with_capacity(f.evaluations.len());
    let mut vals = Vec::with_capacity(f.evaluations.len());
    for (i, v) in f.evaluations.iter() {
        idx.push(*i as u64);
        vals.push(v.to_limbs());
    }
    (idx, vals)
}
fn dense_from_limbs<F: Limbs4>(num_vars: usize, l: &[[u64; 4]]) -> DenseMultilinearExtension<F> {
    DenseMultilinearExtension::from_evaluations_vec(num_vars, l.iter().map(|x| F::from_limbs(*x)).collect())
}

/// `initialize_phase_one` (reference `src/gkr_round_sumcheck/mod.rs:22-42`) -> `(h_g, f1_at_g)`.  The entries of `f1_at_g` are
/// exactly the keys the reference's sparse fold produces, zero-valued ones included.
pub fn initialize_phase_one<F: Limbs4>(f1: &SparseMultilinearExtension<F>, f3: &DenseMultilinearExtension<F>, g: &[F])
                                       -> (DenseMultilinearExtension<F>, SparseMultilinearExtension<F>) {
    let dim = f3.num_vars;
    assert_eq!(f1.num_vars, dim * 3);
    assert_eq!(g.len(), dim);
    let (idx, vals) = sparse_arrays(f1);
    let gl: Vec<[u64; 4]> = g.iter().map(|x| x.to_limbs()).collect();
    let mut h_g = vec![[0u64; 4]; 1 << dim];
    let mut oi = vec![0u64; idx.len().max(1)];
    let mut ov = vec![[0u64; 4]; idx.len().max(1)];
    let mut n1 = 0u64;
    check(unsafe {
        sc_gkr_phase_one(idx.as_ptr(), vals.as_ptr() as *const u64, idx.len() as u64, dim as u32, f3.evaluations.as_ptr() as *const u64,
                         gl.as_ptr() as *const u64, 0, h_g.as_mut_ptr() as *mut u64, oi.as_mut_ptr(), ov.as_mut_ptr() as *mut u64, &mut n1)
    });
    let pairs: Vec<(usize, F)> = (0..n1 as usize).map(|i| (oi[i] as usize, F::from_limbs(ov[i]))).collect();
    (dense_from_limbs(dim, &h_g), SparseMultilinearExtension::from_evaluations(2 * dim, &pairs))
}

/// `initialize_phase_two` (reference `src/gkr_round_sumcheck/mod.rs:57-63`)
pub fn initialize_phase_two<F: Limbs4>(f1_g: &SparseMultilinearExtension<F>, u: &[F]) -> DenseMultilinearExtension<F> {
    assert_eq!(u.len() * 2, f1_g.num_vars);
    let (idx, vals) = sparse_arrays(f1_g);
    let ul: Vec<[u64; 4]> = u.iter().map(|x| x.to_limbs()).collect();
    let mut out = vec![[0u64; 4]; 1 << u.len()];
    check(unsafe { sc_gkr_phase_two(idx.as_ptr(), vals.as_ptr() as *const u64, idx.len() as u64, u.len() as u32, ul.as_ptr() as *const u64, 0, out.as_mut_ptr() as *mut u64) });
    dense_from_limbs(u.len(), &out)
}

/// The two message lists of a `GKRProof` (whose fields are `pub(crate)` in the reference, `data_structures.rs:10-11`).
pub struct HipGKRProof<F: Limbs4> {
    pub phase1_sumcheck_msgs: Vec<ProverMsg<F>>,
    pub phase2_sumcheck_msgs: Vec<ProverMsg<F>>,
    /// the challenges the transcript produced (the verifier's sub-claim point)
    pub u: Vec<F>,
    pub v: Vec<F>,
}

/// The library's own Blake2b512Rng (bit-compatible with `ark_sumcheck::rng::Blake2b512Rng`), for the entry points that run
/// the whole Fiat-Shamir loop inside the library.
pub struct HipRng(*mut sc_rng);
impl HipRng {
    pub fn setup() -> Self {
        HipRng(unsafe { sc_rng_setup() })
    }
    /// `feed(&msg)`: the message's canonical serialisation is absorbed
    pub fn feed<M: CanonicalSerialize>(&mut self, msg: &M) {
        let mut buf = Vec::new();
        msg.serialize_uncompressed(&mut buf).expect("serialising to a Vec cannot fail");
        unsafe { sc_rng_feed_bytes(self.0, buf.as_ptr(), buf.len()) }
    }
}
impl Drop for HipRng {
    fn drop(&mut self) {
        unsafe { sc_rng_free(self.0) }
    }
}

/// `GKRRoundSumcheck::prove` (reference `src/gkr_round_sumcheck/mod.rs:93-139`): sparse fold, scatter, both sumcheck phases and
/// the transcript in ONE FFI call (`sc_gkr_prove`).  `rng` must be in the state the reference's `rng` would be in.
pub fn gkr_prove<F: Limbs4>(rng: &mut HipRng, f1: &SparseMultilinearExtension<F>, f2: &DenseMultilinearExtension<F>, f3: &DenseMultilinearExtension<F>,
                            g: &[F]) -> HipGKRProof<F> {
    assert_eq!(f1.num_vars, 3 * f2.num_vars);
    assert_eq!(f1.num_vars, 3 * f3.num_vars);
    let dim = f2.num_vars;
    assert_eq!(g.len(), dim);
    let (idx, vals) = sparse_arrays(f1);
    let gl: Vec<[u64; 4]> = g.iter().map(|x| x.to_limbs()).collect();
    let mut proof = vec![[0u64; 4]; 2 * dim.max(1) * 3];
    let mut uv = vec![[0u64; 4]; 2 * dim.max(1)];
    check(unsafe {
        sc_gkr_prove(rng.0, idx.as_ptr(), vals.as_ptr() as *const u64, idx.len() as u64, dim as u32, f2.evaluations.as_ptr() as *const u64,
                     f3.evaluations.as_ptr() as *const u64, gl.as_ptr() as *const u64, 0, proof.as_mut_ptr() as *mut u64, uv.as_mut_ptr() as *mut u64)
    });
    let msgs = |off: usize| (0..dim).map(|i| prover_msg(&proof[3 * (off + i)..3 * (off + i) + 3])).collect();
    HipGKRProof {
        phase1_sumcheck_msgs: msgs(0),
        phase2_sumcheck_msgs: msgs(dim),
        u: uv[..dim].iter().map(|l| F::from_limbs(*l)).collect(),
        v: uv[dim..2 * dim].iter().map(|l| F::from_limbs(*l)).collect(),
    }
}

/// One instance of [`gkr_prove_batch`]: what a single [`gkr_prove`] call takes.
pub struct GkrInstance<'a, F: Limbs4> {
    pub rng: &'a mut HipRng,
    pub f1: &'a SparseMultilinearExtension<F>,
    pub f2: &'a DenseMultilinearExtension<F>,
    pub f3: &'a DenseMultilinearExtension<F>,
    pub g: &'a [F],
}

/// `instances.iter_mut().map(GKRRoundSumcheck::prove)` for instances of ONE `dim` in one FFI call (`sc_gkr_prove_batch`).  Small
/// instances (`dim <= 9`) are proved concurrently, a workgroup each, inside one kernel; other shapes are proved one after the other
/// inside the call.  Every proof, `(u, v)` and final transcript state is bit for bit what [`gkr_prove`] gives for that instance.
pub fn gkr_prove_batch<F: Limbs4>(instances: &mut [GkrInstance<F>]) -> Vec<HipGKRProof<F>> {
    if instances.is_empty() {
        return Vec::new();
    }
    let dim = instances[0].f2.num_vars;
    let n = instances.len();
    let mut arrays = Vec::with_capacity(n);
    let mut gls: Vec<Vec<[u64; 4]>> = Vec::with_capacity(n);
    for inst in instances.iter() {
        assert_eq!(inst.f1.num_vars, 3 * dim);
        assert_eq!(inst.f2.num_vars, dim);
        assert_eq!(inst.f3.num_vars, dim);
        assert_eq!(inst.g.len(), dim);
        arrays.push(sparse_arrays(inst.f1));
        gls.push(inst.g.iter().map(|x| x.to_limbs()).collect());
    }
    let rngs: Vec<*mut sc_rng> = instances.iter().map(|i| i.rng.0).collect();
    let idx: Vec<*const u64> = arrays.iter().map(|a| a.0.as_ptr()).collect();
    let vals: Vec<*const u64> = arrays.iter().map(|a| a.1.as_ptr() as *const u64).collect();
    let nnz: Vec<u64> = arrays.iter().map(|a| a.0.len() as u64).collect();
    let f2: Vec<*const u64> = instances.iter().map(|i| i.f2.evaluations.as_ptr() as *const u64).collect();
    let f3: Vec<*const u64> = instances.iter().map(|i| i.f3.evaluations.as_ptr() as *const u64).collect();
    let g: Vec<*const u64> = gls.iter().map(|a| a.as_ptr() as *const u64).collect();
    let rows = dim.max(1);
    let mut proofs = vec![[0u64; 4]; n * 2 * rows * 3];
    let mut uv = vec![[0u64; 4]; n * 2 * rows];
    check(unsafe {
        sc_gkr_prove_batch(n as u32, dim as u32, rngs.as_ptr(), idx.as_ptr(), vals.as_ptr(), nnz.as_ptr(), f2.as_ptr(), f3.as_ptr(), g.as_ptr(), 0,
                           proofs.as_mut_ptr() as *mut u64, uv.as_mut_ptr() as *mut u64)
    });
    (0..n)
        .map(|i| {
            let p = &proofs[i * 2 * dim * 3..(i + 1) * 2 * dim * 3];
            let w = &uv[i * 2 * dim..(i + 1) * 2 * dim];
            let msgs = |off: usize| (0..dim).map(|j| prover_msg(&p[3 * (off + j)..3 * (off + j) + 3])).collect();
            HipGKRProof {
                phase1_sumcheck_msgs: msgs(0),
                phase2_sumcheck_msgs: msgs(dim),
                u: w[..dim].iter().map(|l| F::from_limbs(*l)).collect(),
                v: w[dim..2 * dim].iter().map(|l| F::from_limbs(*l)).collect(),
            }
        })
        .collect()
}

// The batched interactive GKR rounds (`sc_gkr_batch_prover_*`): private declarations behind the safe wrappers below.
extern "C" {
    fn sc_gkr_batch_prover_init(n: u32, dim: u32, f1_idx: *const *const u64, f1_vals: *const *const u64, nnz: *const u64, f2: *const *const u64,
                                f3: *const *const u64, g: *const *const u64, flags: u32, out: *mut *mut sc_gkr_batch_prover) -> c_int;
    fn sc_gkr_batch_prove_round(bp: *mut sc_gkr_batch_prover, r_or_null: *const u64, r_shared: u32, out_evals: *mut u64) -> c_int;
    fn sc_gkr_batch_prover_finish(bp: *mut sc_gkr_batch_prover, r: *const u64, r_shared: u32, out_uv_or_null: *mut u64, out_final_or_null: *mut u64) -> c_int;
    fn sc_gkr_batch_prover_state(bp: *mut sc_gkr_batch_prover, instance: u32, randomness: *mut u64, n_randomness: *mut u32, tables_out: *mut u64,
                                 round: *mut u32) -> c_int;
    fn sc_gkr_batch_prover_reset(bp: *mut sc_gkr_batch_prover) -> c_int;
    fn sc_gkr_batch_prover_free(bp: *mut sc_gkr_batch_prover);
}

/// One instance of [`gkr_prover_init_batch`]: what [`gkr_prove`] takes, without the transcript.
pub struct GkrRoundsInstance<'a, F: Limbs4> {
    pub f1: &'a SparseMultilinearExtension<F>,
    pub f2: &'a DenseMultilinearExtension<F>,
    pub f3: &'a DenseMultilinearExtension<F>,
    pub g: &'a [F],
}

/// n x the two `ProverState`s of `GKRRoundSumcheck::prove` of ONE `dim` behind one `sc_gkr_batch_prover` handle ([`gkr_prover_init_batch`]).
pub struct HipGkrBatchProverState<F: Limbs4> {
    handle: *mut sc_gkr_batch_prover,
    pub n: usize,
    pub dim: usize,
    _f: core::marker::PhantomData<F>,
}

impl<F: Limbs4> Drop for HipGkrBatchProverState<F> {
    fn drop(&mut self) {
        unsafe { sc_gkr_batch_prover_free(self.handle) }
    }
}

impl<F: Limbs4> HipGkrBatchProverState<F> {
    /// round calls answered so far: 0 ..= 2 dim
    pub fn round(&self) -> usize {
        let mut r = 0u32;
        check(unsafe { sc_gkr_batch_prover_state(self.handle, 0, core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut(), &mut r) });
        r as usize
    }
    /// `u` followed by the `v`s instance `i` has received so far
    pub fn randomness(&self, i: usize) -> Vec<F> {
        let mut rand = vec![[0u64; 4]; (2 * self.dim).max(1)];
        let mut n_rand = 0u32;
        check(unsafe { sc_gkr_batch_prover_state(self.handle, i as u32, rand.as_mut_ptr() as *mut u64, &mut n_rand, core::ptr::null_mut(), core::ptr::null_mut()) });
        rand[..n_rand as usize].iter().map(|l| F::from_limbs(*l)).collect()
    }
    /// rewind to round 0 over the inputs the handle holds (phase one's tables are not rebuilt); new inputs: [`gkr_next_layer_batch`]
    pub fn reset(&mut self) {
        check(unsafe { sc_gkr_batch_prover_reset(self.handle) });
    }
}

// An existing handle onto the next layer's inputs (`sc_gkr_layer_next_batch`): a private declaration behind the safe wrapper below.
extern "C" {
    fn sc_gkr_layer_next_batch(bp: *mut sc_gkr_batch_prover, f1_idx_or_null: *const *const u64, f1_vals_or_null: *const *const u64, nnz_or_null: *const u64,
                               f2: *const *const u64, f3: *const *const u64, g: *const *const u64, flags: u32) -> c_int;
}

/// One instance of [`gkr_next_layer_batch`]: the next layer's values and point, and its wiring if it has wiring of its own.
pub struct GkrNextLayerInstance<'a, F: Limbs4> {
    /// `None` for every instance: the wiring the handle holds is kept; `Some` for every instance: new wiring
    pub f1: Option<&'a SparseMultilinearExtension<F>>,
    pub f2: &'a DenseMultilinearExtension<F>,
    pub f3: &'a DenseMultilinearExtension<F>,
    pub g: &'a [F],
}

/// The handle onto the next layer's inputs (`sc_gkr_layer_next_batch`): nothing is allocated, and afterwards the handle is at round 0 as
/// [`gkr_prover_init_batch`] over these inputs would leave it -- same plan, same bits.  Callable in any state.  The inputs are copied; the
/// copy fits whenever the arrays repeat in the pattern init's did and f1 is kept or has no more non-zeros per instance than it had there.
pub fn gkr_next_layer_batch<F: Limbs4>(state: &mut HipGkrBatchProverState<F>, layer: &[GkrNextLayerInstance<F>]) {
    let (n, dim) = (state.n, state.dim);
    assert_eq!(layer.len(), n, "one entry per instance of the handle");
    let keep = layer.iter().all(|i| i.f1.is_none());
    assert!(keep || layer.iter().all(|i| i.f1.is_some()), "new wiring for every instance, or for none");
    let mut arrays = Vec::with_capacity(n);
    let mut gls: Vec<Vec<[u64; 4]>> = Vec::with_capacity(n);
    for inst in layer.iter() {
        assert_eq!(inst.f2.num_vars, dim);
        assert_eq!(inst.f3.num_vars, dim);
        assert_eq!(inst.g.len(), dim);
        if let Some(f1) = inst.f1 {
            assert_eq!(f1.num_vars, 3 * dim);
            arrays.push(sparse_arrays(f1));
        }
        gls.push(inst.g.iter().map(|x| x.to_limbs()).collect());
    }
    let idx: Vec<*const u64> = arrays.iter().map(|a| a.0.as_ptr()).collect();
    let vals: Vec<*const u64> = arrays.iter().map(|a| a.1.as_ptr() as *const u64).collect();
    let nnz: Vec<u64> = arrays.iter().map(|a| a.0.len() as u64).collect();
    let f2: Vec<*const u64> = layer.iter().map(|i| i.f2.evaluations.as_ptr() as *const u64).collect();
    let f3: Vec<*const u64> = layer.iter().map(|i| i.f3.evaluations.as_ptr() as *const u64).collect();
    let g: Vec<*const u64> = gls.iter().map(|a| a.as_ptr() as *const u64).collect();
    let null = core::ptr::null();
    check(unsafe {
        sc_gkr_layer_next_batch(state.handle, if keep { null } else { idx.as_ptr() }, if keep { null } else { vals.as_ptr() },
                                if keep { core::ptr::null() } else { nnz.as_ptr() }, f2.as_ptr(), f3.as_ptr(), g.as_ptr(), 0)
    });
}

// The values of a circuit's layers (`sc_gkr_layers_eval_batch`): a private declaration behind the safe wrapper below.
extern "C" {
    fn sc_gkr_layers_eval_batch(n: u32, dim: u32, n_layers: u32, f1_idx: *const *const u64, f1_vals: *const *const u64, nnz: *const u64,
                                f2: *const *const u64, f3: *const *const u64, flags: u32, out: *const *mut u64) -> c_int;
}

/// The values of a circuit's layers for n instances of ONE `dim` in one FFI call (`sc_gkr_layers_eval_batch`): `f1_layers[k][i]` is the
/// wiring of layer `k` of instance `i`, layer 0 next to the inputs `(f2[i], f3[i])`.  `out[0][i][z]` is the sum over `f1_layers[0][i]`'s
/// non-zeros `(z | x << dim | y << 2 dim, v)` of `v f2[i][x] f3[i][y]`; `out[k][i]` the same over `f1_layers[k][i]` with `out[k-1][i]` on
/// both sides.  The same reference may stand for several instances and layers.  What [`gkr_prover_init_batch`] and
/// [`gkr_next_layer_batch`] take as `f2` and `f3`, layer by layer.
pub fn gkr_evaluate_layers_batch<F: Limbs4>(f1_layers: &[Vec<&SparseMultilinearExtension<F>>], f2: &[&DenseMultilinearExtension<F>],
                                            f3: &[&DenseMultilinearExtension<F>]) -> Vec<Vec<DenseMultilinearExtension<F>>> {
    let (n, n_layers) = (f2.len(), f1_layers.len());
    assert_eq!(f3.len(), n, "one f2 and one f3 per instance");
    if n == 0 || n_layers == 0 {
        return (0..n_layers).map(|_| Vec::new()).collect();
    }
    let dim = f2[0].num_vars;
    let mut arrays = Vec::with_capacity(n * n_layers);
    for layer in f1_layers.iter() {
        assert_eq!(layer.len(), n, "one f1 per layer and instance");
        for f1 in layer.iter() {
            assert_eq!(f1.num_vars, 3 * dim);
            arrays.push(sparse_arrays(*f1));
        }
    }
    for i in 0..n {
        assert_eq!(f2[i].num_vars, dim);
        assert_eq!(f3[i].num_vars, dim);
    }
    let idx: Vec<*const u64> = arrays.iter().map(|a| a.0.as_ptr()).collect();
    let vals: Vec<*const u64> = arrays.iter().map(|a| a.1.as_ptr() as *const u64).collect();
    let nnz: Vec<u64> = arrays.iter().map(|a| a.0.len() as u64).collect();
    let p2: Vec<*const u64> = f2.iter().map(|m| m.evaluations.as_ptr() as *const u64).collect();
    let p3: Vec<*const u64> = f3.iter().map(|m| m.evaluations.as_ptr() as *const u64).collect();
    let mut tables: Vec<Vec<[u64; 4]>> = (0..n * n_layers).map(|_| vec![[0u64; 4]; 1usize << dim]).collect();
    let out: Vec<*mut u64> = tables.iter_mut().map(|t| t.as_mut_ptr() as *mut u64).collect();
    check(unsafe {
        sc_gkr_layers_eval_batch(n as u32, dim as u32, n_layers as u32, idx.as_ptr(), vals.as_ptr(), nnz.as_ptr(), p2.as_ptr(), p3.as_ptr(), 0, out.as_ptr())
    });
    (0..n_layers)
        .map(|k| (0..n).map(|i| DenseMultilinearExtension::from_evaluations_vec(dim, tables[k * n + i].iter().map(|l| F::from_limbs(*l)).collect())).collect())
        .collect()
}

// The two-point form of the handle (`sc_gkr_two_point_init_batch`, `sc_gkr_two_point_next_batch`): private declarations, a block each.
extern "C" {
    fn sc_gkr_two_point_init_batch(n: u32, dim: u32, f1_idx: *const *const u64, f1_vals: *const *const u64, nnz: *const u64, f2: *const *const u64,
                                   f3: *const *const u64, g: *const *const u64, g2: *const *const u64, coef: *const u64, flags: u32,
                                   out: *mut *mut sc_gkr_batch_prover) -> c_int;
}
extern "C" {
    fn sc_gkr_two_point_next_batch(bp: *mut sc_gkr_batch_prover, f1_idx_or_null: *const *const u64, f1_vals_or_null: *const *const u64, nnz_or_null: *const u64,
                                   f2: *const *const u64, f3: *const *const u64, g: *const *const u64, g2: *const *const u64, coef: *const u64,
                                   flags: u32) -> c_int;
}

/// The second point and the coefficients of one instance in two-point form: the handle proves
/// `alpha W(g) + beta W(g2) = sum (alpha f1(g,x,y) + beta f1(g2,x,y)) f2(x) f3(y)`, the claim a GKR layer below the output layer starts from.
pub struct GkrSecondPoint<'a, F: Limbs4> {
    pub g2: &'a [F],
    pub alpha: F,
    pub beta: F,
}

fn second_point_arrays<F: Limbs4>(second: &[GkrSecondPoint<F>], n: usize, dim: usize) -> (Vec<Vec<[u64; 4]>>, Vec<[u64; 4]>) {
    assert_eq!(second.len(), n, "one second point per instance");
    let mut g2s = Vec::with_capacity(n);
    let mut coef = Vec::with_capacity(2 * n);
    for s in second.iter() {
        assert_eq!(s.g2.len(), dim);
        g2s.push(s.g2.iter().map(|x| x.to_limbs()).collect());
        coef.push(s.alpha.to_limbs());
        coef.push(s.beta.to_limbs());
    }
    (g2s, coef)
}

/// [`gkr_prover_init_batch`] in two-point form (`sc_gkr_two_point_init_batch`): `alpha eq(g, .) + beta eq(g2, .)` stands wherever the
/// handle uses `eq(g, .)`; rounds, finish, state and reset are unchanged, and the first value of [`gkr_finish_batch`] is
/// `alpha f1(g,u,v) + beta f1(g2,u,v)`.
pub fn gkr_prover_init_batch_two_point<F: Limbs4>(instances: &[GkrRoundsInstance<F>], second: &[GkrSecondPoint<F>]) -> HipGkrBatchProverState<F> {
    let n = instances.len();
    let dim = if n > 0 { instances[0].f2.num_vars } else { 0 };
    let mut arrays = Vec::with_capacity(n);
    let mut gls: Vec<Vec<[u64; 4]>> = Vec::with_capacity(n);
    for inst in instances.iter() {
        assert_eq!(inst.f1.num_vars, 3 * dim);
        assert_eq!(inst.f2.num_vars, dim);
        assert_eq!(inst.f3.num_vars, dim);
        assert_eq!(inst.g.len(), dim);
        arrays.push(sparse_arrays(inst.f1));
        gls.push(inst.g.iter().map(|x| x.to_limbs()).collect());
    }
    let (g2s, coef) = second_point_arrays(second, n, dim);
    let idx: Vec<*const u64> = arrays.iter().map(|a| a.0.as_ptr()).collect();
    let vals: Vec<*const u64> = arrays.iter().map(|a| a.1.as_ptr() as *const u64).collect();
    let nnz: Vec<u64> = arrays.iter().map(|a| a.0.len() as u64).collect();
    let f2: Vec<*const u64> = instances.iter().map(|i| i.f2.evaluations.as_ptr() as *const u64).collect();
    let f3: Vec<*const u64> = instances.iter().map(|i| i.f3.evaluations.as_ptr() as *const u64).collect();
    let g: Vec<*const u64> = gls.iter().map(|a| a.as_ptr() as *const u64).collect();
    let g2: Vec<*const u64> = g2s.iter().map(|a| a.as_ptr() as *const u64).collect();
    let mut handle: *mut sc_gkr_batch_prover = core::ptr::null_mut();
    check(unsafe {
        sc_gkr_two_point_init_batch(n as u32, dim as u32, idx.as_ptr(), vals.as_ptr(), nnz.as_ptr(), f2.as_ptr(), f3.as_ptr(), g.as_ptr(), g2.as_ptr(),
                                    coef.as_ptr() as *const u64, 0, &mut handle)
    });
    HipGkrBatchProverState { handle, n, dim, _f: core::marker::PhantomData }
}

/// [`gkr_next_layer_batch`] onto a layer in two-point form (`sc_gkr_two_point_next_batch`), on a handle built in either form;
/// [`gkr_next_layer_batch`] afterwards returns the handle to the one-point form.
pub fn gkr_next_layer_batch_two_point<F: Limbs4>(state: &mut HipGkrBatchProverState<F>, layer: &[GkrNextLayerInstance<F>], second: &[GkrSecondPoint<F>]) {
    let (n, dim) = (state.n, state.dim);
    assert_eq!(layer.len(), n, "one entry per instance of the handle");
    let keep = layer.iter().all(|i| i.f1.is_none());
    assert!(keep || layer.iter().all(|i| i.f1.is_some()), "new wiring for every instance, or for none");
    let mut arrays = Vec::with_capacity(n);
    let mut gls: Vec<Vec<[u64; 4]>> = Vec::with_capacity(n);
    for inst in layer.iter() {
        assert_eq!(inst.f2.num_vars, dim);
        assert_eq!(inst.f3.num_vars, dim);
        assert_eq!(inst.g.len(), dim);
        if let Some(f1) = inst.f1 {
            assert_eq!(f1.num_vars, 3 * dim);
            arrays.push(sparse_arrays(f1));
        }
        gls.push(inst.g.iter().map(|x| x.to_limbs()).collect());
    }
    let (g2s, coef) = second_point_arrays(second, n, dim);
    let idx: Vec<*const u64> = arrays.iter().map(|a| a.0.as_ptr()).collect();
    let vals: Vec<*const u64> = arrays.iter().map(|a| a.1.as_ptr() as *const u64).collect();
    let nnz: Vec<u64> = arrays.iter().map(|a| a.0.len() as u64).collect();
    let f2: Vec<*const u64> = layer.iter().map(|i| i.f2.evaluations.as_ptr() as *const u64).collect();
    let f3: Vec<*const u64> = layer.iter().map(|i| i.f3.evaluations.as_ptr() as *const u64).collect();
    let g: Vec<*const u64> = gls.iter().map(|a| a.as_ptr() as *const u64).collect();
    let g2: Vec<*const u64> = g2s.iter().map(|a| a.as_ptr() as *const u64).collect();
    let null = core::ptr::null();
    check(unsafe {
        sc_gkr_two_point_next_batch(state.handle, if keep { null } else { idx.as_ptr() }, if keep { null } else { vals.as_ptr() },
                                    if keep { core::ptr::null() } else { nnz.as_ptr() }, f2.as_ptr(), f3.as_ptr(), g.as_ptr(), g2.as_ptr(),
                                    coef.as_ptr() as *const u64, 0)
    });
}

// The gate form of the handle (`sc_gkr_gates_init_batch`, `sc_gkr_gates_next_batch`): private declarations, a block each.
extern "C" {
    fn sc_gkr_gates_init_batch(n: u32, dim: u32, mul_idx: *const *const u64, mul_vals: *const *const u64, mul_nnz: *const u64, add_idx: *const *const u64,
                               add_vals: *const *const u64, add_nnz: *const u64, f2: *const *const u64, f3: *const *const u64, g: *const *const u64,
                               g2_or_null: *const *const u64, coef_or_null: *const u64, flags: u32, out: *mut *mut sc_gkr_batch_prover) -> c_int;
}
extern "C" {
    fn sc_gkr_gates_next_batch(bp: *mut sc_gkr_batch_prover, mul_idx_or_null: *const *const u64, mul_vals_or_null: *const *const u64, mul_nnz_or_null: *const u64,
                               add_idx_or_null: *const *const u64, add_vals_or_null: *const *const u64, add_nnz_or_null: *const u64, f2: *const *const u64,
                               f3: *const *const u64, g: *const *const u64, g2_or_null: *const *const u64, coef_or_null: *const u64, flags: u32) -> c_int;
}

extern "C" {
    fn sc_gkr_gates_layers_eval_batch(n: u32, dim: u32, n_layers: u32, mul_idx: *const *const u64, mul_vals: *const *const u64, mul_nnz: *const u64,
                                      add_idx: *const *const u64, add_vals: *const *const u64, add_nnz: *const u64, f2: *const *const u64,
                                      f3: *const *const u64, flags: u32, out: *const *mut u64) -> c_int;
}

/// [`gkr_evaluate_layers_batch`] for layers of multiplication and addition gates (`sc_gkr_gates_layers_eval_batch`): `mul_layers[k][i]` and
/// `add_layers[k][i]` are the two lists of layer `k` of instance `i`; `out[k][i][z]` is the sum over `mul` of `v A[x] B[y]` plus the sum
/// over `add` of `v (A[x] + B[y])`, `(A, B) = (f2[i], f3[i])` for layer 0 and `out[k-1][i]` on both sides afterwards.
pub fn gkr_evaluate_layers_batch_gates<F: Limbs4>(mul_layers: &[Vec<&SparseMultilinearExtension<F>>], add_layers: &[Vec<&SparseMultilinearExtension<F>>],
                                                  f2: &[&DenseMultilinearExtension<F>], f3: &[&DenseMultilinearExtension<F>]) -> Vec<Vec<DenseMultilinearExtension<F>>> {
    let (n, n_layers) = (f2.len(), mul_layers.len());
    assert_eq!(f3.len(), n, "one f2 and one f3 per instance");
    assert_eq!(add_layers.len(), n_layers, "one mul and one add list per layer");
    if n == 0 || n_layers == 0 {
        return (0..n_layers).map(|_| Vec::new()).collect();
    }
    let dim = f2[0].num_vars;
    let collect = |layers: &[Vec<&SparseMultilinearExtension<F>>]| {
        let mut arrays = Vec::with_capacity(n * n_layers);
        for layer in layers.iter() {
            assert_eq!(layer.len(), n, "one list per layer and instance");
            for f1 in layer.iter() {
                assert_eq!(f1.num_vars, 3 * dim);
                arrays.push(sparse_arrays(*f1));
            }
        }
        arrays
    };
    let (ma, aa) = (collect(mul_layers), collect(add_layers));
    for i in 0..n {
        assert_eq!(f2[i].num_vars, dim);
        assert_eq!(f3[i].num_vars, dim);
    }
    let mi: Vec<*const u64> = ma.iter().map(|a| a.0.as_ptr()).collect();
    let mv: Vec<*const u64> = ma.iter().map(|a| a.1.as_ptr() as *const u64).collect();
    let mn: Vec<u64> = ma.iter().map(|a| a.0.len() as u64).collect();
    let ai: Vec<*const u64> = aa.iter().map(|a| a.0.as_ptr()).collect();
    let av: Vec<*const u64> = aa.iter().map(|a| a.1.as_ptr() as *const u64).collect();
    let an: Vec<u64> = aa.iter().map(|a| a.0.len() as u64).collect();
    let p2: Vec<*const u64> = f2.iter().map(|m| m.evaluations.as_ptr() as *const u64).collect();
    let p3: Vec<*const u64> = f3.iter().map(|m| m.evaluations.as_ptr() as *const u64).collect();
    let mut tables: Vec<Vec<[u64; 4]>> = (0..n * n_layers).map(|_| vec![[0u64; 4]; 1usize << dim]).collect();
    let out: Vec<*mut u64> = tables.iter_mut().map(|t| t.as_mut_ptr() as *mut u64).collect();
    check(unsafe {
        sc_gkr_gates_layers_eval_batch(n as u32, dim as u32, n_layers as u32, mi.as_ptr(), mv.as_ptr(), mn.as_ptr(), ai.as_ptr(), av.as_ptr(), an.as_ptr(), p2.as_ptr(),
                                       p3.as_ptr(), 0, out.as_ptr())
    });
    (0..n_layers)
        .map(|k| (0..n).map(|i| DenseMultilinearExtension::from_evaluations_vec(dim, tables[k * n + i].iter().map(|l| F::from_limbs(*l)).collect())).collect())
        .collect()
}

/// One instance of a layer of multiplication and addition gates:
/// `W_out[z] = sum over mul of v f2[x] f3[y] + sum over add of v (f2[x] + f3[y])`, claimed at `g`.  `mul` and `add` are `None`
/// together -- only in [`gkr_next_layer_batch_gates`], where that keeps the wiring the handle holds.
pub struct GkrGatesInstance<'a, F: Limbs4> {
    pub mul: Option<&'a SparseMultilinearExtension<F>>,
    pub add: Option<&'a SparseMultilinearExtension<F>>,
    pub f2: &'a DenseMultilinearExtension<F>,
    pub f3: &'a DenseMultilinearExtension<F>,
    pub g: &'a [F],
}

struct GatesArrays {
    lists: Vec<(Vec<u64>, Vec<[u64; 4]>)>, // mul, add per instance
    gls: Vec<Vec<[u64; 4]>>,
    g2s: Vec<Vec<[u64; 4]>>,
    coef: Vec<[u64; 4]>,
}

fn gates_arrays<F: Limbs4>(layer: &[GkrGatesInstance<F>], second: Option<&[GkrSecondPoint<F>]>, dim: usize) -> GatesArrays {
    let n = layer.len();
    let mut a = GatesArrays { lists: Vec::new(), gls: Vec::with_capacity(n), g2s: Vec::new(), coef: Vec::new() };
    for inst in layer.iter() {
        assert_eq!(inst.f2.num_vars, dim);
        assert_eq!(inst.f3.num_vars, dim);
        assert_eq!(inst.g.len(), dim);
        if let (Some(m), Some(d)) = (inst.mul, inst.add) {
            assert_eq!(m.num_vars, 3 * dim);
            assert_eq!(d.num_vars, 3 * dim);
            a.lists.push(sparse_arrays(m));
            a.lists.push(sparse_arrays(d));
        }
        a.gls.push(inst.g.iter().map(|x| x.to_limbs()).collect());
    }
    if let Some(s) = second {
        let (g2s, coef) = second_point_arrays(s, n, dim);
        a.g2s = g2s;
        a.coef = coef;
    }
    a
}

/// [`gkr_prover_init_batch`] for layers of multiplication and addition gates (`sc_gkr_gates_init_batch`), in one-point form or -- with
/// `second` -- in two-point form.  Rounds, reset and state are the handle's; [`gkr_finish_batch`] returns `f2(u)`, `f3(v)` and
/// `f3(v) T1(v) + T2(v)` in the three value fields, the last being what the verifier compares with its expected evaluation; later layers
/// come through [`gkr_next_layer_batch_gates`].
pub fn gkr_prover_init_batch_gates<F: Limbs4>(instances: &[GkrGatesInstance<F>], second: Option<&[GkrSecondPoint<F>]>) -> HipGkrBatchProverState<F> {
    let n = instances.len();
    let dim = if n > 0 { instances[0].f2.num_vars } else { 0 };
    assert!(instances.iter().all(|i| i.mul.is_some() && i.add.is_some()), "init takes both lists of every instance");
    let a = gates_arrays(instances, second, dim);
    let list = |k: usize| -> (Vec<*const u64>, Vec<*const u64>, Vec<u64>) {
        let own: Vec<&(Vec<u64>, Vec<[u64; 4]>)> = a.lists.iter().skip(k).step_by(2).collect();
        (own.iter().map(|l| l.0.as_ptr()).collect(), own.iter().map(|l| l.1.as_ptr() as *const u64).collect(), own.iter().map(|l| l.0.len() as u64).collect())
    };
    let (mi, mv, mn) = list(0);
    let (ai, av, an) = list(1);
    let f2: Vec<*const u64> = instances.iter().map(|i| i.f2.evaluations.as_ptr() as *const u64).collect();
    let f3: Vec<*const u64> = instances.iter().map(|i| i.f3.evaluations.as_ptr() as *const u64).collect();
    let g: Vec<*const u64> = a.gls.iter().map(|x| x.as_ptr() as *const u64).collect();
    let g2: Vec<*const u64> = a.g2s.iter().map(|x| x.as_ptr() as *const u64).collect();
    let mut handle: *mut sc_gkr_batch_prover = core::ptr::null_mut();
    check(unsafe {
        sc_gkr_gates_init_batch(n as u32, dim as u32, mi.as_ptr(), mv.as_ptr(), mn.as_ptr(), ai.as_ptr(), av.as_ptr(), an.as_ptr(), f2.as_ptr(), f3.as_ptr(), g.as_ptr(),
                                if second.is_some() { g2.as_ptr() } else { core::ptr::null() },
                                if second.is_some() { a.coef.as_ptr() as *const u64 } else { core::ptr::null() }, 0, &mut handle)
    });
    HipGkrBatchProverState { handle, n, dim, _f: core::marker::PhantomData }
}

/// [`gkr_next_layer_batch`] for a handle of [`gkr_prover_init_batch_gates`] (`sc_gkr_gates_next_batch`): every instance with both
/// lists (new wiring) or every instance with neither (the handle's wiring is kept); `second` chooses the layer's form.
pub fn gkr_next_layer_batch_gates<F: Limbs4>(state: &mut HipGkrBatchProverState<F>, layer: &[GkrGatesInstance<F>], second: Option<&[GkrSecondPoint<F>]>) {
    let (n, dim) = (state.n, state.dim);
    assert_eq!(layer.len(), n, "one entry per instance of the handle");
    let keep = layer.iter().all(|i| i.mul.is_none() && i.add.is_none());
    assert!(keep || layer.iter().all(|i| i.mul.is_some() && i.add.is_some()), "new wiring for every instance, or for none");
    let a = gates_arrays(layer, second, dim);
    let list = |k: usize| -> (Vec<*const u64>, Vec<*const u64>, Vec<u64>) {
        let own: Vec<&(Vec<u64>, Vec<[u64; 4]>)> = a.lists.iter().skip(k).step_by(2).collect();
        (own.iter().map(|l| l.0.as_ptr()).collect(), own.iter().map(|l| l.1.as_ptr() as *const u64).collect(), own.iter().map(|l| l.0.len() as u64).collect())
    };
    let (mi, mv, mn) = list(0);
    let (ai, av, an) = list(1);
    let f2: Vec<*const u64> = layer.iter().map(|i| i.f2.evaluations.as_ptr() as *const u64).collect();
    let f3: Vec<*const u64> = layer.iter().map(|i| i.f3.evaluations.as_ptr() as *const u64).collect();
    let g: Vec<*const u64> = a.gls.iter().map(|x| x.as_ptr() as *const u64).collect();
    let g2: Vec<*const u64> = a.g2s.iter().map(|x| x.as_ptr() as *const u64).collect();
    let pp = |v: &Vec<*const u64>| if keep { core::ptr::null() } else { v.as_ptr() };
    let pn = |v: &Vec<u64>| if keep { core::ptr::null() } else { v.as_ptr() };
    check(unsafe {
        sc_gkr_gates_next_batch(state.handle, pp(&mi), pp(&mv), pn(&mn), pp(&ai), pp(&av), pn(&an), f2.as_ptr(), f3.as_ptr(), g.as_ptr(),
                                if second.is_some() { g2.as_ptr() } else { core::ptr::null() },
                                if second.is_some() { a.coef.as_ptr() as *const u64 } else { core::ptr::null() }, 0)
    });
}

/// What [`gkr_finish_batch`] returns per instance: the points and the subclaim's oracle values, at no extra pass over the tables.
pub struct GkrBatchFinal<F: Limbs4> {
    pub u: Vec<F>,
    pub v: Vec<F>,
    /// f1(g, u, v)
    pub f1_guv: F,
    /// f2(u)
    pub f2_u: F,
    /// f2(u) f3(v); `f1_guv * f2u_f3v` is what the verifier compares with its expected evaluation
    pub f2u_f3v: F,
}

/// n x the prover of `GKRRoundSumcheck::prove` for instances of ONE `dim` behind one handle (`sc_gkr_batch_prover_init`); every input is copied.
/// `dim <= 9` runs one block per instance; with policy `batch_slices` = 1 (`sc_set_policy`) when the handle is built, `dim` 10 to 16 with at
/// most 64 x 2^dim non-zeros and 16 GiB gives every instance to many blocks (plan `batch.gkr_rounds_slices`: same bits); other shapes take
/// the serial plan.
pub fn gkr_prover_init_batch<F: Limbs4>(instances: &[GkrRoundsInstance<F>]) -> HipGkrBatchProverState<F> {
    let n = instances.len();
    let dim = if n > 0 { instances[0].f2.num_vars } else { 0 };
    let mut arrays = Vec::with_capacity(n);
    let mut gls: Vec<Vec<[u64; 4]>> = Vec::with_capacity(n);
    for inst in instances.iter() {
        assert_eq!(inst.f1.num_vars, 3 * dim);
        assert_eq!(inst.f2.num_vars, dim);
        assert_eq!(inst.f3.num_vars, dim);
        assert_eq!(inst.g.len(), dim);
        arrays.push(sparse_arrays(inst.f1));
        gls.push(inst.g.iter().map(|x| x.to_limbs()).collect());
    }
    let idx: Vec<*const u64> = arrays.iter().map(|a| a.0.as_ptr()).collect();
    let vals: Vec<*const u64> = arrays.iter().map(|a| a.1.as_ptr() as *const u64).collect();
    let nnz: Vec<u64> = arrays.iter().map(|a| a.0.len() as u64).collect();
    let f2: Vec<*const u64> = instances.iter().map(|i| i.f2.evaluations.as_ptr() as *const u64).collect();
    let f3: Vec<*const u64> = instances.iter().map(|i| i.f3.evaluations.as_ptr() as *const u64).collect();
    let g: Vec<*const u64> = gls.iter().map(|a| a.as_ptr() as *const u64).collect();
    let mut handle: *mut sc_gkr_batch_prover = core::ptr::null_mut();
    check(unsafe {
        sc_gkr_batch_prover_init(n as u32, dim as u32, idx.as_ptr(), vals.as_ptr(), nnz.as_ptr(), f2.as_ptr(), f3.as_ptr(), g.as_ptr(), 0, &mut handle)
    });
    HipGkrBatchProverState { handle, n, dim, _f: core::marker::PhantomData }
}

fn gkr_batch_challenges<F: Limbs4>(state: &HipGkrBatchProverState<F>, v_msgs: &[VerifierMsg<F>]) -> (Vec<[u64; 4]>, u32) {
    assert!(v_msgs.len() == state.n || v_msgs.len() == 1, "one VerifierMsg per instance, or a single one for all");
    (v_msgs.iter().map(|m| m.randomness.to_limbs()).collect(), if v_msgs.len() == 1 && state.n != 1 { 1 } else { 0 })
}

/// One round of every instance in one FFI call (`sc_gkr_batch_prove_round`): call it 2 dim times -- phase one's messages, then phase
/// two's.  `None` on the first call, afterwards the previous round's challenges: one per instance, or a single one shared by all.
pub fn gkr_prove_round_batch<F: Limbs4>(state: &mut HipGkrBatchProverState<F>, v_msgs: Option<&[VerifierMsg<F>]>) -> Vec<ProverMsg<F>> {
    let mut out = vec![[0u64; 4]; state.n.max(1) * 3];
    match v_msgs {
        None => check(unsafe { sc_gkr_batch_prove_round(state.handle, core::ptr::null(), 0, out.as_mut_ptr() as *mut u64) }),
        Some(ms) => {
            let (r, shared) = gkr_batch_challenges(state, ms);
            check(unsafe { sc_gkr_batch_prove_round(state.handle, r.as_ptr() as *const u64, shared, out.as_mut_ptr() as *mut u64) })
        }
    }
    (0..state.n).map(|i| prover_msg(&out[3 * i..3 * i + 3])).collect()
}

/// The last challenge `v_{dim-1}` after 2 dim rounds (`sc_gkr_batch_prover_finish`); the handle is exhausted until it is reset.
pub fn gkr_finish_batch<F: Limbs4>(state: &mut HipGkrBatchProverState<F>, v_msgs: &[VerifierMsg<F>]) -> Vec<GkrBatchFinal<F>> {
    let (r, shared) = gkr_batch_challenges(state, v_msgs);
    let (n, dim) = (state.n, state.dim);
    let mut uv = vec![[0u64; 4]; (n * 2 * dim).max(1)];
    let mut fin = vec![[0u64; 4]; n.max(1) * 3];
    check(unsafe { sc_gkr_batch_prover_finish(state.handle, r.as_ptr() as *const u64, shared, uv.as_mut_ptr() as *mut u64, fin.as_mut_ptr() as *mut u64) });
    (0..n)
        .map(|i| {
            let w = &uv[i * 2 * dim..(i + 1) * 2 * dim];
            GkrBatchFinal {
                u: w[..dim].iter().map(|l| F::from_limbs(*l)).collect(),
                v: w[dim..].iter().map(|l| F::from_limbs(*l)).collect(),
                f1_guv: F::from_limbs(fin[3 * i]),
                f2_u: F::from_limbs(fin[3 * i + 1]),
                f2u_f3v: F::from_limbs(fin[3 * i + 2]),
            }
        })
        .collect()
}

/// One instance of [`gkr_verify_subclaim_batch`]: the oracles of a GKR round, the point `g`, and what `GKRRoundSumcheck::verify`
/// returned for its proof.
pub struct GkrSubclaimInstance<'a, F: Limbs4> {
    pub f1: &'a SparseMultilinearExtension<F>,
    pub f2: &'a DenseMultilinearExtension<F>,
    pub f3: &'a DenseMultilinearExtension<F>,
    pub g: &'a [F],
    pub u: &'a [F],
    pub v: &'a [F],
    pub expected_evaluation: F,
}

/// `GKRRoundSumcheckSubClaim::verify_subclaim` (reference `src/gkr_round_sumcheck/data_structures.rs:33-56`) for instances of ONE `dim`
/// in one FFI call (`sc_gkr_subclaim_batch`): `f1(g,u,v) * f2(u) * f3(v) == expected_evaluation` per instance.  What follows
/// [`gkr_prove_batch`] and the verifier -- one more call, not 3 n.
pub fn gkr_verify_subclaim_batch<F: Limbs4>(instances: &[GkrSubclaimInstance<F>]) -> Vec<bool> {
    if instances.is_empty() {
        return Vec::new();
    }
    let dim = instances[0].f2.num_vars;
    let n = instances.len();
    let mut arrays = Vec::with_capacity(n);
    let mut gls: Vec<Vec<[u64; 4]>> = Vec::with_capacity(n);
    let mut uv: Vec<[u64; 4]> = Vec::with_capacity(n * 2 * dim);
    for inst in instances.iter() {
        assert_eq!(inst.f1.num_vars, 3 * dim);
        assert_eq!(inst.f2.num_vars, dim);
        assert_eq!(inst.f3.num_vars, dim);
        assert_eq!(inst.g.len(), dim);
        assert_eq!(inst.u.len(), dim);
        assert_eq!(inst.v.len(), dim);
        arrays.push(sparse_arrays(inst.f1));
        gls.push(inst.g.iter().map(|x| x.to_limbs()).collect());
        uv.extend(inst.u.iter().chain(inst.v.iter()).map(|x| x.to_limbs()));
    }
    let idx: Vec<*const u64> = arrays.iter().map(|a| a.0.as_ptr()).collect();
    let vals: Vec<*const u64> = arrays.iter().map(|a| a.1.as_ptr() as *const u64).collect();
    let nnz: Vec<u64> = arrays.iter().map(|a| a.0.len() as u64).collect();
    let f2: Vec<*const u64> = instances.iter().map(|i| i.f2.evaluations.as_ptr() as *const u64).collect();
    let f3: Vec<*const u64> = instances.iter().map(|i| i.f3.evaluations.as_ptr() as *const u64).collect();
    let g: Vec<*const u64> = gls.iter().map(|a| a.as_ptr() as *const u64).collect();
    let mut evals = vec![[[0u64; 4]; 4]; n];
    check(unsafe {
        sc_gkr_subclaim_batch(n as u32, dim as u32, idx.as_ptr(), vals.as_ptr(), nnz.as_ptr(), f2.as_ptr(), f3.as_ptr(), g.as_ptr(), uv.as_ptr() as *const u64, 0,
                              evals.as_mut_ptr() as *mut u64)
    });
    instances.iter().zip(&evals).map(|(inst, e)| e[3] == inst.expected_evaluation.to_limbs()).collect()
}

// ---- multi-GPU ------------------------------------------------------------------------------------------------------------------
/// One rank of a multi-GPU `MLSumcheck::prove_as_subprotocol` (`sc_ml_prove_sharded`): call it from one thread per GPU after
/// `sc_set_device(rank)`, with `shard` = this rank's contiguous 1/G slice of every table (`num_variables` = the slice's) and a
/// communicator every rank created from the same unique id (`sc_comm_unique_id` on rank 0, `sc_comm_init` everywhere).
/// Returns the proof and the randomness of the GLOBAL instance, identical on every rank.
pub fn prove_sharded<F: Limbs4>(shard: &ListOfProductsOfPolynomials<F>, comm: *mut sc_comm, nv_total: usize) -> (Proof<F>, Vec<F>) {
    let state = prover_init(shard);
    let d = shard.max_multiplicands + 1;
    let mut proof = vec![[0u64; 4]; nv_total * d];
    let mut rand = vec![[0u64; 4]; nv_total];
    check(unsafe { sc_ml_prove_sharded(state.handle, comm, core::ptr::null_mut(), nv_total as u32, proof.as_mut_ptr() as *mut u64, rand.as_mut_ptr() as *mut u64) });
    (proof.chunks(d).map(prover_msg).collect(), rand.iter().map(|l| F::from_limbs(*l)).collect())
}

#[allow(dead_code)]
fn _unused(_: *mut c_void) {}
