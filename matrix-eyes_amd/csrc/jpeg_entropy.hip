// Huffman decoding of sequential JPEG scans on the GPU (csrc/jpeg_entropy.h says how and why the result is exact): what
// crosses to the device is the scan's destuffed bytes and a few KiB of tables, and the coefficients are made there, in the
// layout jpeg_idct_kernel reads.  One thread per subsequence, kThreads subsequences per workgroup; the Huffman tables are
// staged into LDS once per workgroup.  Workgroups meet only at launch boundaries: a sync round is a launch, and the host
// looks at the rounds' changed counts once per batch of launches.  No kernel waits for another workgroup, and every loop
// ends with the bits of its subsequence, so a hostile file costs a bounded number of bounded launches and then declines.
//   jpeg_entropy_speculate_kernel   cold-start decode of every subsequence
//   jpeg_entropy_sync_kernel        one Jacobi round; a workgroup none of whose predecessors changed only copies its states
//   jpeg_entropy_scan_kernel        segmented exclusive sums of blocks / DC differences inside a workgroup, its aggregate
//                                   (the workgroup scan of scan.h over (sums, head flag) pairs)
//   jpeg_entropy_carry_kernel       the aggregates' running sums (one thread: a few hundred workgroups)
//   jpeg_entropy_write_kernel       the true chain: coefficients, and the status word when it meets garbage
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "jpeg_entropy.h"
#include "model.h"
#include "scan.h"

namespace me {

namespace {

using namespace me_jpeg_entropy;

struct Aggregate {
    Counts sum;        // over the workgroup's subsequences behind its last segment head (all of them when it has none)
    int32_t has_head;
};

__global__ __launch_bounds__(kThreads) void jpeg_entropy_speculate_kernel(const Stream st, uint64_t* __restrict__ state0,
                                                                          Counts* __restrict__ counts) {
    __shared__ EntropyTables tab;
    me_scan::stage_to_lds<kThreads>(tab, st.tables);
    const int32_t i = (int32_t)blockIdx.x * kThreads + (int32_t)threadIdx.x;
    if (i < tab.scan.nsub) speculate_thread(tab, st, i, state0, counts);
}

__global__ __launch_bounds__(kThreads) void jpeg_entropy_sync_kernel(const Stream st, const uint64_t* prev, const uint64_t* in,
                                                                     uint64_t* out, Counts* counts, int32_t nsub,
                                                                     int32_t* changed) {
    __shared__ EntropyTables tab;
    const int32_t i = (int32_t)blockIdx.x * kThreads + (int32_t)threadIdx.x;
    // does anybody here decode?  (the first subsequence of a segment never does)
    bool need = false;
    if (i > 0 && i < nsub) need = st.sub_seg[i - 1] == st.sub_seg[i] && !(prev && prev[i - 1] == in[i - 1]);
    if (!__syncthreads_or(need ? 1 : 0)) {
        if (i < nsub) out[i] = in[i];
        return;
    }
    me_scan::stage_to_lds<kThreads>(tab, st.tables);
    if (i < nsub && sync_thread(tab, st, i, prev, in, out, counts)) atomicAdd(changed, 1);
}

__device__ __forceinline__ Counts add_counts(const Counts& a, const Counts& b) {
    Counts r;
    r.blocks = a.blocks + b.blocks;
    r.dc[0] = a.dc[0] + b.dc[0], r.dc[1] = a.dc[1] + b.dc[1], r.dc[2] = a.dc[2] + b.dc[2];
    return r;
}

// a segmented sum as a scan: the sums behind the last segment head, and whether there was a head
struct Seg {
    uint4 sum;  // a Counts (x: blocks, y z w: the DC sums), so that it stays in registers
    uint32_t head;
};
struct SegAdd {
    __device__ Seg operator()(const Seg& a, const Seg& b) const {
        if (b.head) return b;
        return {make_uint4(a.sum.x + b.sum.x, a.sum.y + b.sum.y, a.sum.z + b.sum.z, a.sum.w + b.sum.w), a.head};
    }
};

// before[i]: the sums over the subsequences of i's segment in front of i that lie in i's workgroup
__global__ __launch_bounds__(kThreads) void jpeg_entropy_scan_kernel(const Stream st, const Counts* __restrict__ counts,
                                                                     int32_t nsub, Counts* __restrict__ before,
                                                                     Aggregate* __restrict__ agg) {
    static_assert(sizeof(Counts) == sizeof(uint4), "a Counts is read and written as one uint4");
    __shared__ Seg totals[kThreads / 64];
    const int32_t i = (int32_t)blockIdx.x * kThreads + (int32_t)threadIdx.x;
    Seg mine = {make_uint4(0, 0, 0, 0), 0};
    if (i < nsub) mine = {reinterpret_cast<const uint4*>(counts)[i], st.seg_sub0[st.sub_seg[i]] == i ? 1u : 0u};
    Seg all;
    const Seg front = me_scan::block_scan<kThreads>(mine, totals, all, SegAdd());
    if (i < nsub) reinterpret_cast<uint4*>(before)[i] = mine.head ? make_uint4(0, 0, 0, 0) : front.sum;
    if (threadIdx.x == 0) {
        reinterpret_cast<uint4*>(&agg[blockIdx.x].sum)[0] = all.sum;
        agg[blockIdx.x].has_head = (int32_t)all.head;
    }
}

// carry[g]: the sums over the subsequences in front of workgroup g that belong to the segment running into it
__global__ void jpeg_entropy_carry_kernel(const Aggregate* __restrict__ agg, int32_t ngroups, Counts* __restrict__ carry) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    Counts run = {0, {0, 0, 0}};
    for (int32_t g = 0; g < ngroups; ++g) {
        carry[g] = run;
        run = agg[g].has_head ? agg[g].sum : add_counts(run, agg[g].sum);
    }
}

__global__ __launch_bounds__(kThreads) void jpeg_entropy_write_kernel(const Stream st, const uint64_t* __restrict__ final_state,
                                                                      Counts* before, const Counts* __restrict__ carry,
                                                                      int16_t* __restrict__ coef, int32_t* status) {
    __shared__ EntropyTables tab;
    me_scan::stage_to_lds<kThreads>(tab, st.tables);
    const int32_t group0 = (int32_t)blockIdx.x * kThreads, i = group0 + (int32_t)threadIdx.x;
    if (i >= tab.scan.nsub) return;
    if (st.seg_sub0[st.sub_seg[i]] < group0) before[i] = add_counts(carry[blockIdx.x], before[i]);  // its segment began earlier
    const int err = write_thread(tab, st, i, final_state, before, coef);
    if (err) atomicMax(status, err);
}

}  // namespace

// One attempt at decoding `file`'s scan on the device into the context's "jpeg.coef" buffer.  True: the coefficients are
// there (the stream has been synchronised once, behind the kernels, for the status word) and `plan.frame` describes them;
// false: declined -- ctx->jpeg_entropy_report says why -- and nothing of the file has been judged: the caller runs the host
// decoder, whose result or refusal stands.
bool jpeg_entropy_decode(me_ctx* ctx, const std::vector<uint8_t>& file, int32_t subseq_bits,
                         matrix_eyes::JpegEntropyPlan& plan) {
    using clock = std::chrono::steady_clock;
    JpegEntropyReport& rep = ctx->jpeg_entropy_report;
    rep = JpegEntropyReport();
    ctx->jpeg_entropy_reported = true;
    const int32_t S = subseq_bits ? subseq_bits : kDefaultSubseqBits;
    ME_CHECK(S >= kMinSubseqBits && S <= kMaxSubseqBits && S % 32 == 0, ME_ERR_BAD_ARG,
             "JPEG entropy decoder: %d bits per subsequence (a multiple of 32 in [%d, %d])", S, kMinSubseqBits, kMaxSubseqBits);
    rep.subseq_bits = S;
    hipStream_t s = ctx->stream;
    const auto t0 = clock::now();
    try {
        plan = matrix_eyes::plan_jpeg_entropy(file, "<jpeg>");
    } catch (const matrix_eyes::ImageError&) {
        rep.reason = matrix_eyes::kJpegDeclineHostError;
        return false;
    }
    if (!plan.eligible) {
        rep.reason = plan.reason;
        return false;
    }
    if (!ctx->jpeg_entropy_status)
        ME_HIP(hipHostMalloc((void**)&ctx->jpeg_entropy_status, (kRoundsPerBatch + 1) * sizeof(int32_t), hipHostMallocDefault));
    const size_t cap = upload_capacity(plan, S);
    uint32_t* host = reinterpret_cast<uint32_t*>(jpeg_pinned_buffer(ctx, cap * 2));
    const Layout lay = prepare(plan, file.data(), S, host);
    ME_CHECK(lay.total <= cap, ME_ERR_BAD_ARG, "JPEG entropy decoder: upload of %zu dwords planned as %zu", lay.total, cap);
    rep.ms[0] = std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    const int32_t nsub = lay.nsub, ngroups = (int32_t)cdiv(nsub, kThreads);
    rep.segments = lay.nseg, rep.subseqs = nsub, rep.workgroups = ngroups, rep.upload_bytes = (int64_t)lay.total * 4;
    const int32_t max_rounds = max_sync_rounds(host, lay, S);

    uint32_t* dev = (uint32_t*)site_buf(ctx, "jpeg.entropy.in", lay.total * 4);
    uint64_t* states = (uint64_t*)site_buf(ctx, "jpeg.entropy.states", (size_t)nsub * 3 * sizeof(uint64_t));
    Counts* counts = (Counts*)site_buf(ctx, "jpeg.entropy.counts", (size_t)nsub * sizeof(Counts));
    Counts* before = (Counts*)site_buf(ctx, "jpeg.entropy.before", (size_t)nsub * sizeof(Counts));
    Aggregate* agg = (Aggregate*)site_buf(ctx, "jpeg.entropy.agg", (size_t)ngroups * sizeof(Aggregate));
    Counts* carry = (Counts*)site_buf(ctx, "jpeg.entropy.carry", (size_t)ngroups * sizeof(Counts));
    int32_t* ctl = (int32_t*)site_buf(ctx, "jpeg.entropy.ctl", (size_t)(max_rounds + 2) * sizeof(int32_t));  // status, changed[r]
    const size_t total_coefs = plan.frame.total_coefs;
    int16_t* coef = (int16_t*)site_buf(ctx, "jpeg.coef", total_coefs * sizeof(int16_t));

    ctx->jpeg_entropy_marks.record(0, s);
    ME_HIP(hipMemcpyAsync(dev, host, lay.total * 4, hipMemcpyHostToDevice, s));
    ctx->jpeg_upload.uploaded_on(s);
    ctx->jpeg_entropy_marks.record(1, s);
    ME_HIP(hipMemsetAsync(ctl, 0, (size_t)(max_rounds + 2) * sizeof(int32_t), s));
    ME_HIP(hipMemsetAsync(coef, 0, total_coefs * sizeof(int16_t), s));
    const Stream st = stream_of(dev, lay);
    const dim3 grid((unsigned)ngroups), block(kThreads);
    hipLaunchKernelGGL(jpeg_entropy_speculate_kernel, grid, block, 0, s, st, states, counts);
    ME_HIP(hipGetLastError());
    int32_t round = 0, converged_at = 0;  // rounds launched; the first one without a change
    while (!converged_at && round < max_rounds) {
        const int32_t first = round + 1, n = std::min(kRoundsPerBatch, max_rounds - round);
        for (int32_t q = 0; q < n; ++q) {
            ++round;
            const uint64_t* in = states + (size_t)((round - 1) % 3) * nsub;
            const uint64_t* prev = round >= 2 ? states + (size_t)((round - 2) % 3) * nsub : nullptr;
            hipLaunchKernelGGL(jpeg_entropy_sync_kernel, grid, block, 0, s, st, prev, in, states + (size_t)(round % 3) * nsub, counts,
                               nsub, ctl + round);
            ME_HIP(hipGetLastError());
        }
        ME_HIP(hipMemcpyAsync(ctx->jpeg_entropy_status, ctl + first, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        ME_HIP(hipStreamSynchronize(s));
        for (int32_t q = 0; q < n && !converged_at; ++q)
            if (ctx->jpeg_entropy_status[q] == 0) converged_at = first + q;
    }
    rep.rounds = converged_at ? converged_at : round;
    if (!converged_at) {
        rep.reason = matrix_eyes::kJpegDeclineNoSync;
        return false;
    }
    const uint64_t* final_state = states + (size_t)(round % 3) * nsub;
    hipLaunchKernelGGL(jpeg_entropy_scan_kernel, grid, block, 0, s, st, (const Counts*)counts, nsub, before, agg);
    ME_HIP(hipGetLastError());
    hipLaunchKernelGGL(jpeg_entropy_carry_kernel, dim3(1), dim3(64), 0, s, (const Aggregate*)agg, ngroups, carry);
    ME_HIP(hipGetLastError());
    hipLaunchKernelGGL(jpeg_entropy_write_kernel, grid, block, 0, s, st, final_state, before, (const Counts*)carry, coef, ctl);
    ME_HIP(hipGetLastError());
    ctx->jpeg_entropy_marks.record(2, s);
    ME_HIP(hipMemcpyAsync(ctx->jpeg_entropy_status, ctl, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ME_HIP(hipStreamSynchronize(s));
    rep.ms[1] = ctx->jpeg_entropy_marks.ms(0, 1), rep.ms[2] = ctx->jpeg_entropy_marks.ms(1, 2);
    if (ctx->jpeg_entropy_status[0] != 0) {
        rep.reason = ctx->jpeg_entropy_status[0];
        return false;
    }
    rep.where = 1;
    return true;
}

void free_jpeg_entropy_scratch(me_ctx* ctx) {
    ctx->jpeg_entropy_marks.destroy();
    if (ctx->jpeg_entropy_status) (void)hipHostFree(ctx->jpeg_entropy_status);
    ctx->jpeg_entropy_status = nullptr;
}

}  // namespace me
