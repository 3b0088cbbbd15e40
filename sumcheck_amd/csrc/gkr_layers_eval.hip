// gkr_layers_eval.hip -- sc_gkr_layers_eval_batch: the values of a circuit's layers for n instances of one dim, on the device -- what the
// sc_gkr_batch_prover_* family (gkr_batch_rounds.hip) consumes as f2 and f3, layer by layer.  Inputs and wiring go in, every layer's values
// stay on the device (SC_TABLES_ON_DEVICE: written in place), and the handle walks back over them.  Two plans, chosen per call, same bits
// (kernels_batch_gkr_eval_layers.hip):
//   batch.gkr_eval_layers_one_block  dim <= 9, every list of every layer within 64 x 2^dim, policy "batch" != 0: ONE launch for all layers;
//   batch.gkr_eval_cells             everything else: per layer the cells zeroed, k_batch_gkr_eval_terms, k_batch_gkr_eval_fold on one stream.
// One upload (records | output pointers | index flags), for device-resident lists the index check over ALL layers in front of the first
// launch that follows indices, the launches, for host arrays the copies back, one synchronisation.  The work area -- the image, the staged
// host arrays, the cells -- is process-wide and kept between calls (sc_set_cache_limit, sc_release_caches); one call at a time holds it.
#include "batch_slices.hpp"
#include "prover_internal.hpp"

namespace {

struct EvalLayersArea {
    std::mutex mu;
    int device = -1;
    hipStream_t stream = nullptr;
    char *d_buf = nullptr, *h_pin = nullptr;
    size_t d_cap = 0, pin_cap = 0;
    void free_all() {
        if (device >= 0) (void)hipSetDevice(device);
        if (d_buf) (void)hipFree(d_buf);
        if (h_pin) (void)hipHostFree(h_pin);
        if (stream) (void)hipStreamDestroy(stream);
        (void)hipGetLastError();
        d_buf = h_pin = nullptr;
        stream = nullptr;
        d_cap = pin_cap = 0;
        device = -1;
    }
};
EvalLayersArea g_eval_area;

// at least d_bytes of device memory and pin_bytes of pinned host memory on device dev, with the area's stream (the caller holds the area and the gate)
int area_reserve(EvalLayersArea &a, int dev, size_t d_bytes, size_t pin_bytes) {
    HIP_TRY(hipSetDevice(dev));
    if (a.device != dev) {
        a.free_all();
        HIP_TRY(hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking));
        a.device = dev;
    }
    if (a.d_cap < d_bytes) {
        if (a.d_buf) (void)hipFree(a.d_buf);
        a.d_buf = nullptr;
        a.d_cap = 0;
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&a.d_buf), d_bytes));
        a.d_cap = d_bytes;
    }
    if (a.pin_cap < pin_bytes) {
        if (a.h_pin) (void)hipHostFree(a.h_pin);
        a.h_pin = nullptr;
        a.pin_cap = 0;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&a.h_pin), pin_bytes, hipHostMallocDefault));
        a.pin_cap = pin_bytes;
    }
    return SC_OK;
}

struct Range {
    uintptr_t b, e;
};
// does [b, e) meet a range of `sorted` (by begin; pre[k]: the largest end among the first k + 1)?  skip: the position of the range itself, or -1
bool meets(const std::vector<Range> &sorted, const std::vector<uintptr_t> &pre, uintptr_t b, uintptr_t e, ptrdiff_t skip) {
    const size_t k = std::lower_bound(sorted.begin(), sorted.end(), e, [](const Range &r, uintptr_t v) { return r.b < v; }) - sorted.begin(); // ranges [0, k) begin below e
    if (skip < 0) return k > 0 && pre[k - 1] > b;
    // the range's own place is among [0, k): whatever begins before it and reaches beyond b, or begins behind it and below e
    if (skip > 0 && pre[(size_t)skip - 1] > b) return true;
    return (size_t)skip + 1 < k;
}

} // namespace

void sc_internal_release_gkr_eval_cache() {
    std::lock_guard<std::mutex> lk(g_eval_area.mu);
    g_eval_area.free_all();
}

namespace {
// sc_gkr_layers_eval_batch (add_idx, add_vals and add_nnz null: multiplication gates only, errors name the list f1) and
// sc_gkr_gates_layers_eval_batch (an ADD list beside every MUL list, errors name mul or add): the same checks, the same image with the ADD
// records behind the MUL records, the same work area; the gate form launches kernels_batch_gkr_gates.hip's kernels and counts its own plans
int eval_layers(uint32_t n, uint32_t dim, uint32_t n_layers, const uint64_t *const *f1_idx, const uint64_t *const *f1_vals, const uint64_t *nnz, const uint64_t *const *add_idx,
                const uint64_t *const *add_vals, const uint64_t *add_nnz, const uint64_t *const *f2, const uint64_t *const *f3, uint32_t flags, uint64_t *const *out);
} // namespace

extern "C" int sc_gkr_layers_eval_batch(uint32_t n, uint32_t dim, uint32_t n_layers, const uint64_t *const *f1_idx, const uint64_t *const *f1_vals, const uint64_t *nnz,
                                        const uint64_t *const *f2, const uint64_t *const *f3, uint32_t flags, uint64_t *const *out) {
    return eval_layers(n, dim, n_layers, f1_idx, f1_vals, nnz, nullptr, nullptr, nullptr, f2, f3, flags, out);
}

// sc_gkr_layers_eval_batch with both lists per (layer, instance): W_out[z] = sum_MUL v A[x] B[y] + sum_ADD v (A[x] + B[y])
extern "C" int sc_gkr_gates_layers_eval_batch(uint32_t n, uint32_t dim, uint32_t n_layers, const uint64_t *const *mul_idx, const uint64_t *const *mul_vals, const uint64_t *mul_nnz,
                                              const uint64_t *const *add_idx, const uint64_t *const *add_vals, const uint64_t *add_nnz, const uint64_t *const *f2,
                                              const uint64_t *const *f3, uint32_t flags, uint64_t *const *out) {
    if (n == 0 || n_layers == 0) return SC_OK;
    if (!add_idx || !add_vals || !add_nnz) return sc_internal_fail(SC_ERR_BAD_ARG, "layer 0 instance 0: null argument");
    return eval_layers(n, dim, n_layers, mul_idx, mul_vals, mul_nnz, add_idx, add_vals, add_nnz, f2, f3, flags, out);
}

namespace {
int eval_layers(uint32_t n, uint32_t dim, uint32_t n_layers, const uint64_t *const *f1_idx, const uint64_t *const *f1_vals, const uint64_t *nnz, const uint64_t *const *add_idx,
                const uint64_t *const *add_vals, const uint64_t *add_nnz, const uint64_t *const *f2, const uint64_t *const *f3, uint32_t flags, uint64_t *const *out) {
    if (n == 0 || n_layers == 0) return SC_OK;
    const bool gates = add_idx != nullptr;
    const char *const mul_name = gates ? "mul" : "f1";
    // ---- everything the host can check, before any HIP call: the lowest failing (layer, instance) decides ----
    if (!f1_idx || !f1_vals || !nnz || !f2 || !f3 || !out) return sc_internal_fail(SC_ERR_BAD_ARG, "layer 0 instance 0: null argument");
    if (dim == 0) return sc_internal_fail(SC_ERR_CONSTANT_POLY, "layer 0 instance 0: Attempt to prove a constant.");
    if (dim > 21) return sc_internal_fail(SC_ERR_BAD_ARG, "layer 0 instance 0: dim %u: 3*dim index bits do not fit 64-bit indices", dim);
    const bool dev_in = flags & SC_TABLES_ON_DEVICE;
    const size_t N = (size_t)1 << dim, tab_bytes = N * 32, total = (size_t)n_layers * n;
    // the ranges of every input (each distinct one once) and of every output, sorted by their begin
    std::vector<Range> ins, outs;
    {
        std::map<std::pair<uintptr_t, uintptr_t>, int> seen;
        auto add = [&](const void *p, size_t bytes) {
            if (!p || bytes == 0) return;
            const uintptr_t b = reinterpret_cast<uintptr_t>(p);
            if (seen.emplace(std::make_pair(b, b + bytes), 0).second) ins.push_back({b, b + bytes});
        };
        for (size_t r = 0; r < total; ++r) {
            if (nnz[r] >= (1ULL << 31)) continue; // (refused below)
            add(f1_idx[r], (size_t)nnz[r] * 8);
            add(f1_vals[r], (size_t)nnz[r] * 32);
            if (gates && add_nnz[r] < (1ULL << 31)) {
                add(add_idx[r], (size_t)add_nnz[r] * 8);
                add(add_vals[r], (size_t)add_nnz[r] * 32);
            }
        }
        for (uint32_t i = 0; i < n; ++i) {
            add(f2[i], tab_bytes);
            add(f3[i], tab_bytes);
        }
        for (size_t r = 0; r < total; ++r)
            if (out[r]) outs.push_back({reinterpret_cast<uintptr_t>(out[r]), reinterpret_cast<uintptr_t>(out[r]) + tab_bytes});
    }
    auto by_begin = [](const Range &a, const Range &b) { return a.b < b.b || (a.b == b.b && a.e < b.e); };
    std::sort(ins.begin(), ins.end(), by_begin);
    std::sort(outs.begin(), outs.end(), by_begin);
    auto prefix = [](const std::vector<Range> &v) {
        std::vector<uintptr_t> pre(v.size());
        uintptr_t m = 0;
        for (size_t k = 0; k < v.size(); ++k) pre[k] = m = std::max(m, v[k].e);
        return pre;
    };
    const std::vector<uintptr_t> ins_pre = prefix(ins), outs_pre = prefix(outs);
    uint64_t nnz_all = 0;
    std::vector<uint64_t> nnz_layer(n_layers, 0);
    for (uint32_t k = 0; k < n_layers; ++k)
        for (uint32_t i = 0; i < n; ++i) {
            const size_t r = (size_t)k * n + i;
            if (nnz[r] >= (1ULL << 31)) return sc_internal_fail(SC_ERR_BAD_ARG, "layer %u instance %u: nnz too large (a list holds fewer than 2^31 non-zeros)", k, i);
            if (gates && (add_nnz[r] >= (1ULL << 31) || nnz[r] + add_nnz[r] >= (1ULL << 31)))
                return sc_internal_fail(SC_ERR_BAD_ARG, "layer %u instance %u: nnz too large (the two lists together hold fewer than 2^31 non-zeros)", k, i);
            if ((nnz[r] && (!f1_idx[r] || !f1_vals[r])) || (k == 0 && (!f2[i] || !f3[i])) || !out[r]) return sc_internal_fail(SC_ERR_BAD_ARG, "layer %u instance %u: null argument", k, i);
            if (gates && add_nnz[r] && (!add_idx[r] || !add_vals[r])) return sc_internal_fail(SC_ERR_BAD_ARG, "layer %u instance %u: null argument", k, i);
            const uintptr_t ob = reinterpret_cast<uintptr_t>(out[r]), oe = ob + tab_bytes;
            if (meets(ins, ins_pre, ob, oe, -1)) return sc_internal_fail(SC_ERR_BAD_ARG, "layer %u instance %u: the output overlaps an input", k, i);
            const ptrdiff_t self = std::lower_bound(outs.begin(), outs.end(), Range{ob, oe}, by_begin) - outs.begin();
            if (meets(outs, outs_pre, ob, oe, self)) return sc_internal_fail(SC_ERR_BAD_ARG, "layer %u instance %u: the output overlaps another output", k, i);
            if (!dev_in)
                for (uint64_t t = 0; t < nnz[r]; ++t)
                    if ((f1_idx[r][t] >> (3 * dim)) != 0) return sc_internal_fail(SC_ERR_BAD_ARG, "layer %u instance %u: %s has an index out of range", k, i, mul_name);
            if (!dev_in && gates)
                for (uint64_t t = 0; t < add_nnz[r]; ++t)
                    if ((add_idx[r][t] >> (3 * dim)) != 0) return sc_internal_fail(SC_ERR_BAD_ARG, "layer %u instance %u: add has an index out of range", k, i);
            const uint64_t longest = gates ? std::max(nnz[r], add_nnz[r]) : nnz[r];
            nnz_layer[k] = std::max(nnz_layer[k], longest);
            nnz_all = std::max(nnz_all, longest);
        }
    const bool one_block = scd::policy(scd::kPolBatch) != 0 && scd::gkr_batch_shape_fits(dim, nnz_all);
    const uint64_t cells_bytes = one_block ? 0 : ((uint64_t)n * scd::kBsGkrCellBytes) << dim;
    if (cells_bytes > scd::kBsMaxWorkBytes)
        return sc_internal_fail(SC_ERR_OOM, "the cells of %u instances of dim %u take %llu bytes, beyond the work area's 16 GiB: evaluate fewer instances per call", n, dim,
                                (unsigned long long)cells_bytes);
    if (sc_device_count() <= 0) return sc_internal_fail(SC_ERR_HIP, "no HIP device visible: libsumcheck_hip has no CPU fallback");

    // ---- the image: records | output pointers | index flags; behind it on the device the staged host arrays and outputs, then the cells ----
    const size_t rec_off = 0, out_off = rec_off + round_up((add_idx ? 2 : 1) * total * sizeof(scd::GkrBatchInst), 256), flag_off = out_off + round_up(total * sizeof(void *), 256);
    const size_t n_rec = gates ? 2 * total : total; // (gate form: the ADD records behind the MUL records, and their flags behind the MUL records' flags)
    const size_t image_bytes = flag_off + round_up(n_rec * 4, 256);
    StageMap st;
    st.align = 256;
    st.base = image_bytes;
    std::vector<size_t> offs, add_offs; // host arrays: per record idx, vals; then per instance f2, f3; (gate form) per record the ADD list's idx, vals
    if (!dev_in && gates) {
        add_offs.resize(2 * total);
        for (size_t r = 0; r < total; ++r) {
            add_offs[2 * r + 0] = add_nnz[r] ? st.add(add_idx[r], (size_t)add_nnz[r] * 8) : st.base;
            add_offs[2 * r + 1] = add_nnz[r] ? st.add(add_vals[r], (size_t)add_nnz[r] * 32) : st.base;
        }
    }
    if (!dev_in) {
        offs.resize(2 * total + 2 * (size_t)n);
        for (size_t r = 0; r < total; ++r) {
            offs[2 * r + 0] = nnz[r] ? st.add(f1_idx[r], (size_t)nnz[r] * 8) : st.base;
            offs[2 * r + 1] = nnz[r] ? st.add(f1_vals[r], (size_t)nnz[r] * 32) : st.base;
        }
        for (uint32_t i = 0; i < n; ++i) {
            offs[2 * total + 2 * (size_t)i + 0] = st.add(f2[i], tab_bytes);
            offs[2 * total + 2 * (size_t)i + 1] = st.add(f3[i], tab_bytes);
        }
    }
    const size_t stage_out_off = st.base + st.bytes, stage_out_bytes = dev_in ? 0 : total * round_up(tab_bytes, 256);
    const size_t cells_off = stage_out_off + stage_out_bytes, d_bytes = cells_off + (size_t)cells_bytes;

    const int dev = sc_internal_device_ref();
    std::lock_guard<std::mutex> lease(g_eval_area.mu);
    EvalLayersArea &a = g_eval_area;
    auto run = [&]() -> int {
        DeviceGate gate_(dev);
        if (int rc = area_reserve(a, dev, d_bytes, image_bytes)) return rc;
        if (dev_in) HIP_TRY(hipDeviceSynchronize()); // the inputs' producers are waited for, as a copy on their stream would
        char *const d_up = a.d_buf;
        auto d_out = [&](size_t r) { return dev_in ? reinterpret_cast<char *>(out[r]) : d_up + stage_out_off + r * round_up(tab_bytes, 256); };
        scd::GkrBatchInst *rec = reinterpret_cast<scd::GkrBatchInst *>(a.h_pin + rec_off);
        void **outp = reinterpret_cast<void **>(a.h_pin + out_off);
        std::memset(a.h_pin + flag_off, 0, image_bytes - flag_off);
        for (uint32_t k = 0; k < n_layers; ++k)
            for (uint32_t i = 0; i < n; ++i) {
                const size_t r = (size_t)k * n + i;
                scd::GkrBatchInst &R = rec[r];
                R.nnz = nnz[r];
                R.g = nullptr;
                R.idx = dev_in ? f1_idx[r] : reinterpret_cast<const uint64_t *>(d_up + offs[2 * r + 0]);
                R.vals = reinterpret_cast<const uint4 *>(dev_in ? reinterpret_cast<const char *>(f1_vals[r]) : d_up + offs[2 * r + 1]);
                if (k == 0) {
                    R.f2 = reinterpret_cast<const uint4 *>(dev_in ? reinterpret_cast<const char *>(f2[i]) : d_up + offs[2 * total + 2 * (size_t)i + 0]);
                    R.f3 = reinterpret_cast<const uint4 *>(dev_in ? reinterpret_cast<const char *>(f3[i]) : d_up + offs[2 * total + 2 * (size_t)i + 1]);
                } else {
                    R.f2 = R.f3 = reinterpret_cast<const uint4 *>(d_out(r - n)); // the layer before, on both sides
                }
                outp[r] = d_out(r);
                if (gates) { // (the ADD record: its list; the tables are read through the MUL record)
                    scd::GkrBatchInst &D = rec[total + r];
                    D = R;
                    D.nnz = add_nnz[r];
                    D.idx = dev_in ? add_idx[r] : reinterpret_cast<const uint64_t *>(d_up + add_offs[2 * r + 0]);
                    D.vals = reinterpret_cast<const uint4 *>(dev_in ? reinterpret_cast<const char *>(add_vals[r]) : d_up + add_offs[2 * r + 1]);
                }
            }
        HIP_TRY(hipMemcpyAsync(d_up, a.h_pin, image_bytes, hipMemcpyHostToDevice, a.stream));
        for (const StageMap::Item &it : st.items) HIP_TRY(hipMemcpyAsync(d_up + it.off, it.src, it.bytes, hipMemcpyHostToDevice, a.stream));
        const scd::GkrBatchInst *d_rec = reinterpret_cast<const scd::GkrBatchInst *>(d_up + rec_off);
        // device-resident lists: an index out of range is found here, over all layers, in front of the first launch that follows indices
        if (dev_in)
            for (size_t first = 0; first < n_rec; first += 1u << 30) { // (the check's n is 32 bits wide)
                const uint32_t count = (uint32_t)std::min<size_t>(n_rec - first, 1u << 30);
                HIP_TRY(scd::launch_batch_gkr_idx_range(d_rec + first, count, dim, reinterpret_cast<uint32_t *>(d_up + flag_off) + first, a.stream));
            }
        if (dev_in) {
            HIP_TRY(hipMemcpyAsync(a.h_pin + flag_off, d_up + flag_off, n_rec * 4, hipMemcpyDeviceToHost, a.stream));
            HIP_TRY(hipStreamSynchronize(a.stream));
            const uint32_t *fl = reinterpret_cast<const uint32_t *>(a.h_pin + flag_off);
            for (size_t r = 0; r < total; ++r) { // (the lowest failing (layer, instance) decides, mul before add)
                if (fl[r]) return sc_internal_fail(SC_ERR_BAD_ARG, "layer %u instance %u: %s has an index out of range", (uint32_t)(r / n), (uint32_t)(r % n), mul_name);
                if (gates && fl[total + r]) return sc_internal_fail(SC_ERR_BAD_ARG, "layer %u instance %u: add has an index out of range", (uint32_t)(r / n), (uint32_t)(r % n));
            }
        }
        scd::GkrEvalLayersArgs A;
        std::memset(&A, 0, sizeof(A));
        A.n = n;
        A.dim = dim;
        if (one_block) {
            A.inst = d_rec;
            A.out = reinterpret_cast<uint4 *const *>(d_up + out_off);
            A.n_layers = n_layers;
            if (gates) HIP_TRY(scd::launch_batch_gkr_gates_eval_layers(scd::GkrGatesEvalArgs{A, d_rec + total}, a.stream));
            else HIP_TRY(scd::launch_batch_gkr_eval_layers(A, a.stream));
        } else {
            A.cells = reinterpret_cast<uint64_t *>(d_up + cells_off);
            A.n_layers = 1;
            for (uint32_t k = 0; k < n_layers; ++k) {
                A.inst = d_rec + (size_t)k * n;
                A.out = reinterpret_cast<uint4 *const *>(d_up + out_off) + (size_t)k * n;
                HIP_TRY(hipMemsetAsync(A.cells, 0, (size_t)cells_bytes, a.stream));
                if (gates) HIP_TRY(scd::launch_batch_gkr_gates_eval_cells(scd::GkrGatesEvalArgs{A, d_rec + total + (size_t)k * n}, nnz_layer[k], a.stream));
                else HIP_TRY(scd::launch_batch_gkr_eval_cells(A, nnz_layer[k], a.stream));
            }
        }
        if (!dev_in)
            for (size_t r = 0; r < total; ++r) HIP_TRY(hipMemcpyAsync(out[r], d_out(r), tab_bytes, hipMemcpyDeviceToHost, a.stream));
        HIP_TRY(hipStreamSynchronize(a.stream));
        return SC_OK;
    };
    const int rc = run();
    // a HIP error leaves no stream with work behind and nothing cached; an argument refusal (the device's index check) keeps the area for the
    // caller's next call; over the cache limit nothing is kept between calls
    if ((rc != SC_OK && rc != SC_ERR_BAD_ARG) || a.d_cap > sc_internal_cache_limit()) {
        const std::string why = rc ? sc_last_error() : "";
        {
            DeviceGate gate_(dev);
            if (a.stream) (void)hipStreamSynchronize(a.stream);
            a.free_all();
        }
        if (rc) return sc_internal_fail(rc, "%s", why.c_str());
    }
    if (rc) return rc;
    if (gates) scd::plan_hit(one_block ? scd::kPlanBatchGkrGatesEvalOneBlock : scd::kPlanBatchGkrGatesEvalCells);
    else scd::plan_hit(one_block ? scd::kPlanBatchGkrEvalLayersOneBlock : scd::kPlanBatchGkrEvalLayersCells);
    return SC_OK;
}
} // namespace
