// Tile-configuration choice and (dtype, A-mode, epilogue) dispatch for the GEMM core.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>

#include "gemm_core.h"

#include "admission.h"  // (behind the HIP headers: tile_choice.h states its functions for both sides under hipcc)

namespace me {

void fail(int32_t code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw Error{code, buf};
}

// explicit specialisations live in gemm_{f16,bf16}_{plain,conv}.hip
#define ME_DECL(T, A, E) \
    template <>          \
    void gemm_dispatch<T, A, E>(const GemmParams&, int, hipStream_t);
ME_DECL(f16, A_PLAIN, EPI_STORE)
ME_DECL(f16, A_PLAIN, EPI_RESID_SCALE)
ME_DECL(f16, A_PLAIN, EPI_PATCH_EMBED)
ME_DECL(f16, A_PLAIN, EPI_CONVT)
ME_DECL(f16, A_CONV, EPI_STORE)
ME_DECL(f16, A_CONV, EPI_HEAD_FINAL)
ME_DECL(bf16, A_PLAIN, EPI_STORE)
ME_DECL(bf16, A_PLAIN, EPI_RESID_SCALE)
ME_DECL(bf16, A_PLAIN, EPI_PATCH_EMBED)
ME_DECL(bf16, A_PLAIN, EPI_CONVT)
ME_DECL(bf16, A_CONV, EPI_STORE)
ME_DECL(bf16, A_CONV, EPI_HEAD_FINAL)
#undef ME_DECL

static thread_local unsigned* g_status_word = nullptr;
unsigned* current_status_word() { return g_status_word; }
void set_current_status_word(unsigned* w) { g_status_word = w; }

Profiler& profiler() {
    static thread_local Profiler p;
    return p;
}
ProfScope::ProfScope(hipStream_t s, const std::string& name, double flops, double bytes) : stream(s) {
    Profiler& p = profiler();
    if (!p.enabled) return;
    ProfEntry e;
    e.name = name, e.flops = flops, e.bytes = bytes;
    if (hipEventCreate(&e.e0) != hipSuccess || hipEventCreate(&e.e1) != hipSuccess) return;
    (void)hipEventRecord(e.e0, stream);
    index = (int)p.entries.size();
    p.entries.push_back(e);
}
ProfScope::~ProfScope() {
    if (index >= 0) (void)hipEventRecord(profiler().entries[index].e1, stream);
}

int gemm_num_configs() { return CFG_COUNT; }
const char* gemm_config_name(int cfg) { return cfg >= 0 && cfg < CFG_COUNT ? kTileConfigs[cfg].name : "?"; }

// The knobs of tile_choice.h's rules, read once per process (ME_FP8_TALL is not among them: gemm_fp8.hip reads it per launch).
const TileKnobs& tile_knobs() {
    static const TileKnobs knobs = [] {
        TileKnobs k;
        k.dynamic_tiles = getenv("ME_GEMM_DYNAMIC_TILES") != nullptr;
        k.conv_halo = env_on("ME_CONV_HALO"), k.conv_halo12 = env_on("ME_CONV_HALO12"), k.conv_halo128 = env_on("ME_CONV_HALO128");
        k.tall = env_on("ME_GEMM_TALL");
        k.tall_bias = getenv("ME_GEMM_TALL_BIAS") ? atof(getenv("ME_GEMM_TALL_BIAS")) : 0.95;
        k.tail96 = env_on("ME_GEMM_TAIL96");
        k.pp192 = getenv("ME_GEMM_PP192") != nullptr;
        k.split_k = env_flag("ME_SPLIT_K");
        k.split_k_min_k = env_int("ME_SPLIT_K_MINK", 4096);  // (the tests lower it: a tiny model has no K that deep)
        return k;
    }();
    return knobs;
}

static TileProblem tile_problem(const GemmParams& p, AMode amode, EpiKind epi) {
    return {p.M, p.N, p.K, p.seg1, p.seg2, amode, epi, p.KH, p.KW, p.stride, p.out_H, p.out_W, p.Cin, p.tap_bias != nullptr, p.ln_out16 != nullptr,
            p.A2 != nullptr};
}

template <typename T>
static void launch_typed(const GemmParams& p, AMode amode, EpiKind epi, int cfg, hipStream_t s) {
    if (amode == A_PLAIN) {
        switch (epi) {
            case EPI_STORE: gemm_dispatch<T, A_PLAIN, EPI_STORE>(p, cfg, s); return;
            case EPI_RESID_SCALE: gemm_dispatch<T, A_PLAIN, EPI_RESID_SCALE>(p, cfg, s); return;
            case EPI_PATCH_EMBED: gemm_dispatch<T, A_PLAIN, EPI_PATCH_EMBED>(p, cfg, s); return;
            case EPI_CONVT: gemm_dispatch<T, A_PLAIN, EPI_CONVT>(p, cfg, s); return;
            default: break;
        }
    } else {
        switch (epi) {
            case EPI_STORE: gemm_dispatch<T, A_CONV, EPI_STORE>(p, cfg, s); return;
            case EPI_HEAD_FINAL: gemm_dispatch<T, A_CONV, EPI_HEAD_FINAL>(p, cfg, s); return;
            default: break;
        }
    }
    fail(ME_ERR_BAD_ARG, "gemm: unsupported (A-mode %d, epilogue %d)", (int)amode, (int)epi);
}

// One tile-queue block per launch stream (kernels of a stream run one after the other; the last
// workgroup of a launch leaves the counters zeroed for the next).
static unsigned* queue_for_stream(hipStream_t stream) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, unsigned*> blocks;
    int dev = 0;
    ME_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    unsigned*& q = blocks[{dev, stream}];
    if (!q) {
        ME_HIP(hipMalloc((void**)&q, kGemmQueueWords * sizeof(unsigned)));
        ME_HIP(hipMemset(q, 0, kGemmQueueWords * sizeof(unsigned)));
    }
    return q;
}

// Compute units a stream may use.  A stream created with hipExtStreamCreateWithCUMask (or a process under a global CU
// mask) gets fewer than the device reports; a persistent grid sized from the device's count would then queue workgroups
// behind one another -- harmless for the plain kernels, a wait without partner for the fused LayerNorm launch.
int stream_cu_count(hipStream_t stream) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, int> cache;
    int dev = 0;
    ME_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find({dev, stream});
    if (it != cache.end()) return it->second;
    int cus = 0;
    ME_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    int granted = cus;
    uint32_t mask[32] = {0};
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool capturing = stream && hipStreamIsCapturing(stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
    if (!capturing && hipExtStreamGetCUMask(stream, 32, mask) == hipSuccess) {
        int bits = 0;
        for (uint32_t w : mask) bits += __builtin_popcount(w);
        if (bits > 0 && bits < cus) granted = bits;
    }
    (void)hipGetLastError();
    if (!capturing) cache[{dev, stream}] = granted;
    return granted;
}

// ME_LOG_LAUNCH: one line per launch on stderr -- which shape a trace row is
static bool log_launches() { static const bool on = getenv("ME_LOG_LAUNCH") != nullptr; return on; }
// ME_GEMM_GRID_LIMIT, a diagnostic (tools/dual_stream_probe.py): cap the persistent grid of the two-group launchers (gemm_core.h
// gemm_launch_pp, gemm_fp8.hip launch_pp8t) so that two launches on two streams share the chip instead of the first one taking
// every CU until it ends.  On the fused LayerNorm launch a cap that is not a whole number of rounds' units puts column tiles of one
// row tile into different rounds: the waits run into their bound and raise ME_STATUS_SYNC_TIMEOUT -- which is how
// tests/test_gpu_pipeline.py forces the fallback path.
int gemm_grid_limit() { static const int limit = env_int("ME_GEMM_GRID_LIMIT", 0); return limit; }
// ME_LN_SPIN_LIMIT, the same test's other knob: the polls of GemmParams::ln_spin_limit
int gemm_ln_spin_limit() { static const int spin = env_int("ME_LN_SPIN_LIMIT", 0); return spin > 0 ? spin : 0; }

void head_composed_launch_f16(const GemmParams& p, hipStream_t stream);
void head_composed_launch_bf16(const GemmParams& p, hipStream_t stream);

void head_composed_launch(const GemmParams& p_in, int32_t dtype, hipStream_t stream) {
    GemmParams p = p_in;
    p.resident_out = nullptr, p.queue = nullptr, p.status = current_status_word();
    p.cu_granted = stream_cu_count(stream);
    admit_head_composed(p);
    if (log_launches()) fprintf(stderr, "gemm_launch conv head_composed M=%d N=%d K=%d\n", p.M, p.N, p.K);
    // algorithmic FLOPs: every output phase reads a 2 x 2 window of the 3 x 3 one (4 of 9 taps carry weights): the dense launch
    // executes 9 / 4 of them; counted here are the FLOPs of the two layers it replaces at their own shapes (SURVEY App. B:
    // ConvTranspose 2 * H * W * Cin * Cin * 4 + conv3x3 2 * 4 H W * Cin * 32 * 9)
    const double px = (double)p.M;
    ProfScope prof(stream, std::string("gemm_kernel<") + (dtype == ME_DTYPE_F16 ? "f16" : "bf16") + ",16x16px-x128x64/8w-halo,conv,head_composed>",
                   2.0 * px * p.Cin * p.Cin * 4 + 2.0 * 4 * px * p.Cin * 32 * 9,
                   px * p.Cin * 2 + (double)p.N * p.K * 2 + 4 * px * 4);
    if (dtype == ME_DTYPE_F16) head_composed_launch_f16(p, stream);
    else if (dtype == ME_DTYPE_BF16) head_composed_launch_bf16(p, stream);
    else fail(ME_ERR_BAD_ARG, "composed head: bad dtype %d", dtype);
}

int gemm_lnf_resident(int32_t dtype, hipStream_t stream) {
    GemmParams p = GemmParams();
    int32_t resident = 0;
    p.resident_out = &resident;
    p.cu_granted = stream_cu_count(stream);
    p.ln_out16 = &resident;  // (selects the LNF instantiation; nothing is launched)
    p.K = 128;
    if (dtype == ME_DTYPE_F16)
        gemm_dispatch<f16, A_PLAIN, EPI_RESID_SCALE>(p, CFG_PP352, stream);
    else if (dtype == ME_DTYPE_BF16)
        gemm_dispatch<bf16, A_PLAIN, EPI_RESID_SCALE>(p, CFG_PP352, stream);
    else
        fail(ME_ERR_BAD_ARG, "gemm: bad dtype %d", dtype);
    return resident;
}

void gemm_launch(const GemmParams& p_in, AMode amode, EpiKind epi, int32_t dtype, hipStream_t stream,
                 int32_t force_cfg) {
    GemmParams p = p_in;
    p.resident_out = nullptr;
    p.cu_granted = stream_cu_count(stream);
    p.ln_spin_limit = gemm_ln_spin_limit();
    // Dynamic tile order (TileQueue in gemm_core.h) is an opt-in: measured on the full step it gains 0.4 %
    // (26.57 vs 26.68 ms) -- the launches the side streams disturb most (proj / fc2) have two tiles per
    // workgroup, too coarse for a late workgroup to hand work to its neighbours.
    p.queue = tile_knobs().dynamic_tiles ? queue_for_stream(stream) : nullptr;
    p.status = current_status_word();
    p.gelu_per_granule = !env_on("ME_GELU_BATCH");  // (read per launch: the tests flip it inside one process)
    static const int patch_rows = env_int("ME_GEMM_PATCH_ROWS", 0);  // A/B knob
    p.patch_rows = patch_rows;
    admit_gemm(p, amode, epi);  // (admission.h)
    if (p.A2) p.queue = nullptr;  // (a chained operand set runs the static tile order: a pass is not a tile the queue could hand out)
    // which tile, and whether it takes this problem (tile_choice.h): nothing is launched on a refusal
    const TileProblem problem = tile_problem(p, amode, epi);
    const int cfg = resolve_config(problem, force_cfg, tile_knobs());
    if (const TileRefusal no = config_refusal(problem, cfg); no.kind != TILE_OK)
        fail(no.kind == TILE_BAD_SHAPE ? ME_ERR_BAD_SHAPE : ME_ERR_BAD_ARG, "gemm: tile config %d (%s), %s M=%d N=%d K=%d, row segments %d / %d: %s", cfg,
             gemm_config_name(cfg), amode == A_CONV ? "conv" : "plain", p.M, p.N, p.K, p.seg1, p.seg2, no.why);
    static const char* kEpi[] = {"store", "resid_scale", "patch_embed", "?", "convt", "head_final"};
    // the head's final layers on a halo tile (head_conv.hip) where the shape is the model's own; force_cfg >= 0 or
    // ME_HEAD_HALO=0: the implicit-GEMM tile below
    static const bool head_halo_on = env_on("ME_HEAD_HALO");
    const bool head_halo = epi == EPI_HEAD_FINAL && amode == A_CONV && force_cfg < 0 && head_halo_on && head_final_halo_fits(p);
    if (log_launches())
        fprintf(stderr, "gemm_launch %s %s M=%d N=%d K=%d k=%dx%d/s%d cfg=%s res32=%d out32=%d out16=%d border=%d lo=%d hi2=%d ln=%d wrap=%d K2=%d\n",
                amode == A_PLAIN ? "plain" : "conv", kEpi[epi], p.M, p.N, p.K, p.KH, p.KW, p.stride, gemm_config_name(cfg),
                p.res32 != nullptr, p.out32 != nullptr, p.out16 != nullptr, p.out16_border, (int)p.lo_off16, (int)p.hi2_off16,
                p.ln_out16 != nullptr, p.a_wrap, p.A2 ? p.K2 : 0);
    // algorithmic bytes of the launch (every operand once): what an HBM-bound launch is priced against in bench.py's
    // kernels[] (the MFMA fraction misstates the residual launches and the ConvTransposes)
    double launch_bytes = 0.0;
    {
        const double MN = (double)p.M * p.N;
        // (a wrapped row is read as far as it is stored; a chained launch reads both operand sets)
        launch_bytes += amode == A_PLAIN ? (double)p.M * (p.a_wrap ? p.a_wrap * 64 : p.K) * 2                 // activation rows
                                         : (double)p.M * (p.stride > 0 ? p.stride * p.stride : 1) * p.Cin * 2;  // input pixels, once
        launch_bytes += (double)p.N * p.K * 2;
        if (p.A2) launch_bytes += (double)p.M * (p.a_wrap2 ? p.a_wrap2 * 64 : p.K2) * 2 + (double)p.N * p.K2 * 2;
        if (epi == EPI_HEAD_FINAL) launch_bytes += (double)p.M * 4;
        else {
            if (p.out16) launch_bytes += MN * 2 * (1 + (p.lo_off16 ? 1 : 0) + (p.hi2_off16 ? 1 : 0));
            if (p.out32) launch_bytes += MN * 4;
            if (p.res32) launch_bytes += MN * 4;
            if (p.res32b) launch_bytes += MN * 4;
            if (p.ln_out16) launch_bytes += p.out8 ? MN : MN * 2;
            else if (p.out8) launch_bytes += MN;
        }
    }
    ProfScope prof(stream,
                   std::string("gemm_kernel<") + (dtype == ME_DTYPE_F16 ? "f16" : "bf16") + "," +
                       (head_halo ? "12x16px-x32/8w-halo" : (epi == EPI_HEAD_FINAL ? "256x32x64/4w" : gemm_config_name(cfg))) + "," +
                       (amode == A_PLAIN ? "plain" : "conv") + "," + kEpi[epi] + ">",
                   2.0 * (p.flop_rows ? p.flop_rows : p.M) * p.N * ((p.flop_k ? p.flop_k : p.K) + (p.A2 ? (p.flop_k2 ? p.flop_k2 : p.K2) : 0)),
                   launch_bytes);
    if (head_halo) {
        head_final_halo_launch(p, dtype, stream);
        return;
    }
    if (dtype == ME_DTYPE_F16)
        launch_typed<f16>(p, amode, epi, cfg, stream);
    else if (dtype == ME_DTYPE_BF16)
        launch_typed<bf16>(p, amode, epi, cfg, stream);
    else
        fail(ME_ERR_BAD_ARG, "gemm: bad dtype %d", dtype);
}

}  // namespace me
