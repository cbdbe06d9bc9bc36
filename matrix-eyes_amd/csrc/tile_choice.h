// Which tile a GEMM or convolution runs on: the configuration ids, one table of what each configuration is and admits, and the launch
// decisions of gemm_launch (gemm.hip), the ViT linears (pipeline.hip) and the fp8 GEMM (gemm_fp8.hip) as pure functions of the problem
// and the knobs.  Free of HIP and of getenv, so that a host compiler alone can build and test it (tests/test_tile_choice_cpu.py);
// the .hip side fills TileKnobs (gemm.hip tile_knobs) and raises what config_refusal answers.  DESIGN.md 4.39.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ME_TILE_FN __host__ __device__ __forceinline__
#else
#define ME_TILE_FN inline
#endif

namespace me {

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

enum AMode : int32_t {
    A_PLAIN = 0,  // A row-major [M][lda]
    A_CONV = 1    // A gathered from a zero-bordered NHWC map: row m = (b,y,x), k = (tap, cin)
};

enum EpiKind : int32_t {
    EPI_STORE = 0,       // out32 [M][ldc] / out16 (row-major, or pixels of a zero-bordered NHWC
                         // map when out16_border) = act(acc + bias + res32 + res32b)
    EPI_RESID_SCALE = 1, // out32[m][n] = res32[m][n] + gamma[n]*(acc + bias[n])  (ViT proj / fc2)
    EPI_PATCH_EMBED = 2, // out32[(m/P)*(P+1) + 1 + m%P][n] = acc + bias[n] + pos[1 + m%P][n]
    EPI_CONVT = 4,       // ConvTranspose2d(2,2,s2) pixel shuffle: n = (dy*2+dx)*Cout + co
    EPI_HEAD_FINAL = 5,  // relu(acc+bias) . w2 + b2 -> relu -> / f_norm -> clamp  (N <= 32)
    EPI_HEAD_COMPOSED = 6 // the same behind the composed ConvTranspose o conv3x3 of the head (weights.hip compose_head): N = 4
                          // output phases x 32 channels on the half-resolution map, out32 = the full-resolution depth
};

// Workgroups per round of every cost model below: the MI355X's 256 compute units, one workgroup of a two-group kernel on each.  The
// models do NOT follow a stream's CU mask or a smaller part (launch_grid.h sizes the grids from those; the choice of tile does not).
constexpr int kRoundWorkgroups = 256;

// row tiles of a launch tiled per row segment (gemm_core.h seg_tile_rows; the 352-row tile)
template <int BM>
ME_TILE_FN int seg_row_tiles(int M, int seg1, int seg2) {
    if (seg1 == 0) return (M + BM - 1) / BM;
    const int e1 = seg2 ? seg2 : M;
    return (seg1 + BM - 1) / BM + (e1 - seg1 + BM - 1) / BM + (seg2 ? (M - seg2 + BM - 1) / BM : 0);
}

// ---- the configurations ---------------------------------------------------------------------------------
// The ids are what me_op_* take as tile_cfg (ABI); a negative id asks for the automatic choice.
enum { CFG_PP256 = 0, CFG_128 = 1, CFG_64 = 2, CFG_160 = 3, CFG_RING64 = 4, CFG_PP192 = 5, CFG_8PH = 6, CFG_PP96 = 7,
       CFG_RING128 = 8, CFG_HALO = 9, CFG_PP352 = 10, CFG_HALO12 = 11, CFG_HALO_N128 = 12, CFG_COUNT = 13 };

constexpr uint32_t pair_bit(int amode, int epi) { return 1u << (amode * 8 + epi); }
constexpr uint32_t kPlainLinear = pair_bit(A_PLAIN, EPI_STORE) | pair_bit(A_PLAIN, EPI_RESID_SCALE);
constexpr uint32_t kConvStore = pair_bit(A_CONV, EPI_STORE);
// every pair ME_GEMM_DISPATCH_BODY is instantiated for (gemm_*_{plain,conv}.hip).  (A_CONV, EPI_HEAD_FINAL) is not among them: its
// dispatch is one kernel whatever the id (config_refusal)
constexpr uint32_t kAnyPair = kPlainLinear | pair_bit(A_PLAIN, EPI_PATCH_EMBED) | pair_bit(A_PLAIN, EPI_CONVT) | kConvStore;

struct TileConfig {
    const char* name;  // as the profiler and ME_LOG_LAUNCH report it
    int rows, cols;    // of the output tile (halo tiles: pixels x channels)
    int seg_align;     // row segments must start on multiples of it; 1: any boundary will do (the 352-row tile lays its row tiles
                       // out per segment, gemm_core.h seg_tile_rows; a convolution on the 12-row halo tile has no segments)
    bool two_slab;     // prefetches two K slabs ahead: K >= 128, a shorter K runs on CFG_128
    uint32_t admits;   // pair_bit(A-mode, epilogue) of the instantiations gemm_core.h ME_GEMM_DISPATCH_BODY compiles for it
    bool cf_modes;     // its kernel compiles the bordered and tap-bias epilogue modes (gemm_core.h gemm_epilogue CF_MODES)
};
constexpr TileConfig kTileConfigs[CFG_COUNT] = {
    /* CFG_PP256     */ {"256x256x64/8w-pp", 256, 256, 256, true, kAnyPair, true},
    /* CFG_128       */ {"128x128x64/4w", 128, 128, 128, false, kAnyPair, true},
    /* CFG_64        */ {"64x64x64/4w", 64, 64, 64, false, kAnyPair, true},
    /* CFG_160       */ {"160x128x64/4w", 160, 128, 160, false, kAnyPair, true},
    /* CFG_RING64    */ {"64x64x64/4w-ring6", 64, 64, 64, false, kAnyPair, true},
    /* CFG_PP192     */ {"192x256x64/8w-pp", 192, 256, 192, true, kAnyPair, true},
    /* CFG_8PH       */ {"256x256x64/8w-8ph", 256, 256, 256, true, kPlainLinear, true},
    /* CFG_PP96      */ {"96x256x64/8w-pp", 96, 256, 96, true, kPlainLinear | kConvStore, true},
    /* CFG_RING128   */ {"128x256x64/8w-ring3", 128, 256, 128, false, kPlainLinear | kConvStore, true},
    /* CFG_HALO      */ {"16x16px-x256x64/8w-halo", 256, 256, 256, false, kConvStore, true},
    /* CFG_PP352     */ {"352x256x64/8w-pp", 352, 256, 1, true, kPlainLinear, false},
    /* CFG_HALO12    */ {"12x16px-x256x64/8w-halo", 192, 256, 1, false, kConvStore, true},
    /* CFG_HALO_N128 */ {"16x16px-x128x64/8w-halo", 256, 128, 256, false, kConvStore, true},
};
constexpr bool tile_admits(int cfg, int amode, int epi) {
    return cfg >= 0 && cfg < CFG_COUNT && (kTileConfigs[cfg].admits & pair_bit(amode, epi)) != 0;
}

// ---- the problem and the knobs --------------------------------------------------------------------------
struct TileProblem {
    int32_t M, N, K, seg1, seg2;
    int32_t amode, epi;  // AMode, EpiKind
    int32_t KH, KW, stride, out_H, out_W, Cin;  // A_CONV
    bool tap_bias;   // GemmParams::tap_bias is set: the launch needs the tap-bias epilogue mode
    bool ln_out16;   // GemmParams::ln_out16 is set: the launch is the fused residual + LayerNorm
    bool chained = false;  // GemmParams::A2 is set: two ConvTransposes summed in one accumulator (gemm_core.h gemm_pp_kernel<..., CHAIN>)
};

// The environment knobs the decisions read, as the .hip side found them (the header never asks the environment).
struct TileKnobs {
    bool dynamic_tiles = false;  // ME_GEMM_DYNAMIC_TILES (set)
    bool conv_halo = true;       // ME_CONV_HALO (=0: off)
    bool conv_halo12 = true;     // ME_CONV_HALO12 (=0: off)
    bool conv_halo128 = true;    // ME_CONV_HALO128 (=0: off)
    bool tall = true;            // ME_GEMM_TALL (=0: no 352-row tile, and with it no fused LayerNorm)
    double tall_bias = 0.95;     // ME_GEMM_TALL_BIAS
    bool tail96 = true;          // ME_GEMM_TAIL96 (=0: off)
    bool pp192 = false;          // ME_GEMM_PP192 (set)
    bool split_k = false;        // ME_SPLIT_K (non-zero: on)
    int split_k_min_k = 4096;    // ME_SPLIT_K_MINK
};
// (ME_FP8_TALL is the one knob read per launch -- the tests flip it inside one process --, so it is fp8_tall_wins' own argument and not a
// member of what is read once)

// ---- gemm_launch: the automatic choice ------------------------------------------------------------------
// Tile choice.  The persistent kernels run ceil(tiles / resident workgroups) rounds, so the cost of a
// configuration is rounds x (tile area) x (workgroups sharing a CU) / (its main-loop efficiency relative
// to the two-group 256x256 kernel, measured at M = 80780 where rounds do not matter: profiles/
// r01_kernel_microbench_f16.json).  Examples at M = 20195: qkv / fc1 (N = 3072 / 4096) -> 256x256 (4 and
// 5 rounds); proj / fc2 (N = 1024) -> 160x128: 1016 tiles = 2 rounds of 512, where 128x128 needs 3 and
// 256x256 leaves 3/4 of the second round idle; the 256-channel convolutions at 768^2 and 384^2 -> 256x256.
// The 64x64 tile is for the single-window ViTs (M = 577) and the low-resolution decoder levels.
inline int pick_config(int64_t M, int64_t N, int64_t K, int64_t seg1, int64_t seg2, bool resid, bool dynamic_tile_order) {
    const int64_t t1 = cdiv(M, 128) * cdiv(N, 128);
    if (N < 128 || t1 < kRoundWorkgroups) {
        // few 64x64 tiles and a long K (the M = 577 fc2: 160 tiles x 64 slabs): the six-slot ring keeps
        // five slabs in flight (33 -> 19 us); with many tiles its 96 KiB of LDS per workgroup costs more
        // in occupancy than the latency it hides
        return cdiv(M, 64) * cdiv(N, 64) <= 512 && K >= 2048 ? CFG_RING64 : CFG_64;
    }
    struct Cand {
        int cfg, per_cu;
        double eff;
    };
    // 192x256 (residual epilogue only): at M = 21760, N = 1024 it turns 340 tiles (1.33 rounds of 256) into 432 (1.69
    // rounds).  Measured standalone: proj (K = 1024) 94.7 -> 80.3 us, fc2 (K = 4096) 229 -> 252 us -- the shorter
    // tile moves 17 % more operand bytes per MFMA through L2 -> LDS and a K = 4096 main loop pays for that, a
    // K = 1024 one is half epilogue and gains from the rounds.
    const Cand cands[] = {{CFG_PP256, 1, 1.0}, {CFG_PP192, 1, K <= 1024 ? 0.88 : 0.68}, {CFG_160, 2, 0.80}, {CFG_128, 2, 0.76}};
    int best = CFG_128;
    double best_cost = 0.0;
    for (const Cand& c : cands) {
        const int bm = kTileConfigs[c.cfg].rows, bn = kTileConfigs[c.cfg].cols;
        if (c.cfg == CFG_PP192 && !resid) continue;
        if (N < bn || (kTileConfigs[c.cfg].two_slab && K < 128)) continue;
        if (seg1 % bm || seg2 % bm) continue;  // row segments must start on tile boundaries
        const int64_t tiles = cdiv(M, bm) * cdiv(N, bn);
        // static order: whole rounds; dynamic order: workgroups draw tiles until none are left, so the
        // launch takes the average share plus about half a tile of tail
        const double rounds = dynamic_tile_order && tiles > kRoundWorkgroups * c.per_cu
                                  ? (double)tiles / ((double)kRoundWorkgroups * c.per_cu) + 0.5
                                  : (double)cdiv(tiles, (int64_t)kRoundWorkgroups * c.per_cu);
        const double cost = rounds * bm * bn * c.per_cu / c.eff;
        if (best_cost == 0.0 || cost < best_cost) best = c.cfg, best_cost = cost;
    }
    return best;
}

// a 3x3 stride-1 convolution with the store epilogue on a map of tile_h x 16 pixel tiles, N a multiple of bn: what a halo tile takes
inline bool halo_fits(const TileProblem& q, int tile_h, int bn) {
    return q.amode == A_CONV && q.epi == EPI_STORE && q.KH == 3 && q.KW == 3 && q.stride == 1 && q.out_H % tile_h == 0 &&
           q.out_W % 16 == 0 && q.N % bn == 0;
}

// The configuration a launch runs on: the forced one, or pick_config's and its halo promotions; then the K < 128 demotion.
inline int resolve_config(const TileProblem& q, int force_cfg, const TileKnobs& knobs) {
    int cfg = force_cfg >= 0 ? force_cfg : pick_config(q.M, q.N, q.K, q.seg1, q.seg2, q.amode == A_PLAIN && q.epi == EPI_RESID_SCALE,
                                                       knobs.dynamic_tiles);
    // 3x3 convolutions big enough for the 256x256 tile take its halo form (gemm_core.h conv_halo_kernel): the 18 x 18
    // halo of a 16 x 16 pixel tile staged once per 64 input channels instead of the pixels once per tap
    if (force_cfg < 0 && knobs.conv_halo && halo_fits(q, 16, 256) && cfg == CFG_PP256) {
        cfg = CFG_HALO;
        // 12-row tiles where they fill the rounds better: a tile of 12 x 16 pixels costs about 0.78 of a 16 x 16 one
        // (three quarters of the MFMAs, the same weight staging per slab)
        if (knobs.conv_halo12 && q.out_H % 12 == 0) {
            const int64_t nbn = q.N / 256, t16 = (int64_t)(q.M / 256) * nbn, t12 = (int64_t)(q.M / 192) * nbn;
            if ((double)cdiv(t12, kRoundWorkgroups) * 0.78 < (double)cdiv(t16, kRoundWorkgroups) * 0.97) cfg = CFG_HALO12;
        }
    }
    // N = 128 (the head's first convolution, 256 -> 128 at 768 x 768): the halo tile with 128 channels where the
    // 128x128 implicit-GEMM tile would have been chosen on a map of at least a round of pixel tiles
    if (force_cfg < 0 && knobs.conv_halo && knobs.conv_halo128 && halo_fits(q, 16, 128) && q.N % 256 != 0 && cfg == CFG_128 &&
        (int64_t)(q.M / 256) * (q.N / 128) >= kRoundWorkgroups)
        cfg = CFG_HALO_N128;
    if (cfg >= 0 && cfg < CFG_COUNT && kTileConfigs[cfg].two_slab && q.K < 128) cfg = CFG_128;  // they prefetch two slabs ahead
    return cfg;
}

// Why a resolved configuration does not take the problem, or TILE_OK.  The launcher raises ME_ERR_BAD_SHAPE / ME_ERR_BAD_ARG for it
// before anything is launched.
enum TileRefusalKind { TILE_OK = 0, TILE_BAD_SHAPE, TILE_BAD_ARG };
struct TileRefusal {
    TileRefusalKind kind;
    const char* why;
};
inline TileRefusal config_refusal(const TileProblem& q, int cfg) {
    if (q.chained && !(cfg == CFG_PP256 && q.amode == A_PLAIN && q.epi == EPI_CONVT))
        return {TILE_BAD_ARG, "a chained operand set takes the 256x256 two-group tile's ConvTranspose form"};
    if (q.ln_out16 && !(cfg == CFG_PP352 && q.amode == A_PLAIN && q.epi == EPI_RESID_SCALE))
        return {TILE_BAD_ARG, "the fused LayerNorm takes the 352-row tile's residual epilogue (K >= 128)"};
    if (cfg == CFG_HALO && !halo_fits(q, 16, 256))
        return {TILE_BAD_SHAPE, "the halo tile takes 3x3 stride-1 convolutions on maps of 16-pixel multiples, N a multiple of 256"};
    if (cfg == CFG_HALO_N128 && !halo_fits(q, 16, 128))
        return {TILE_BAD_SHAPE, "the 128-channel halo tile takes 3x3 stride-1 convolutions on maps of 16-pixel multiples, N a multiple of 128"};
    if (cfg == CFG_HALO12 && !halo_fits(q, 12, 256))
        return {TILE_BAD_SHAPE, "the 12-row halo tile takes 3x3 stride-1 convolutions on maps of 12 x 16 pixel multiples, N a multiple of 256"};
    // the head's final layers: one 256x32 kernel whatever the id says (gemm_*_conv.hip); a forced id only means "not head_conv.hip's"
    const bool one_kernel = q.amode == A_CONV && q.epi == EPI_HEAD_FINAL;
    if (!one_kernel && (cfg < 0 || cfg >= CFG_COUNT)) return {TILE_BAD_ARG, "no such tile configuration"};
    const int bm = one_kernel ? 256 : kTileConfigs[cfg].seg_align;
    if (q.seg1 % bm != 0 || q.seg2 % bm != 0 || !(q.seg2 == 0 || q.seg2 > q.seg1))
        return {TILE_BAD_ARG, "row segments do not start on its tile boundaries"};
    if (!one_kernel && !tile_admits(cfg, q.amode, q.epi)) return {TILE_BAD_ARG, "the configuration is not compiled for this (A-mode, epilogue)"};
    if (q.tap_bias && !one_kernel && !kTileConfigs[cfg].cf_modes)
        return {TILE_BAD_ARG, "the configuration's kernel does not compile the tap-bias epilogue mode"};
    return {TILE_OK, nullptr};
}

// ---- the ViT linears (pipeline.hip gemm_all / resid_all) ------------------------------------------------
// Whole rounds + a short tail.  A persistent 256x256 launch runs ceil(tiles / 256) rounds, and at one image the last
// round of fc1 (1360 tiles: 5.31 rounds) and of proj / fc2 (340 tiles: 1.33 rounds) is a third full.  The main loops
// are bound by what a CU can stage into LDS per slab ((BM + BN) x 128 bytes at ~50 GB/s per CU), not by the MFMAs,
// so a 96x256 tile costs 0.69 of a 256x256 tile's main loop and 0.375 of its epilogue: when the last round is at
// most half full, its rows run as a SECOND launch of 96-row tiles (CFG_PP96; <= 256 of them, one short round
// in which every workgroup has a tile) behind the whole rounds.  The rows of the second launch all belong to the
// last row segment.  Results are bit-identical (same K order per output element).  Measured at one image, FOV head:
// proj 93.7 -> 82.7 us, fc2 211.7 -> 207.7 us stand-alone (profiles/r03_tail_tile_ab.txt); in the step, same box,
// alternating runs: 25.17 ms (off) -> 24.90 (proj / fc2 split) -> 24.70 (fc1 too).  ME_GEMM_TAIL96=0 turns it off.
// Returns the rows of the first launch (pipeline.hip launch_with_short_tail slices the descriptor there), 0: one launch.
inline int64_t short_tail_rows1(int64_t M, int64_t N, int64_t K, int64_t seg1, int64_t seg2, const TileKnobs& knobs) {
    if (!knobs.tail96 || N % 256 || M % 256 || K < 128) return 0;
    const int64_t nbn = N / 256;
    if (kRoundWorkgroups % nbn) return 0;
    const int64_t per_round = kRoundWorkgroups / nbn, row_tiles = M / 256;  // row tiles per round of workgroups
    const int64_t rounds = row_tiles / per_round, rem = row_tiles % per_round;
    const int64_t rows1 = rounds * per_round * 256, rows2 = M - rows1;
    const int64_t last_seg = seg2 ? seg2 : seg1;
    if (rounds < 1 || rem == 0 || 2 * rem > per_round || cdiv(rows2, 96) * nbn > kRoundWorkgroups || rows1 < last_seg) return 0;
    return rows1;
}

// The 352-row tile (CFG_PP352).  256 CUs x one tile each cover 64 x 352 = 22528 rows of an N = 1024 launch: at
// one image proj / fc2 are ONE exact round (3 + 3 + 58 row tiles x 4 = 256 tiles) instead of a round of 256x256
// tiles and a second launch of short tiles that the CU cannot stage fast enough (1.375 tile-times against 1 + 0.69),
// and fc1 is four rounds instead of five and a tail.  Chosen when its rounds x 352 undercut what the 256-row path
// costs (whole rounds x 256, + 0.69 x 256 for a short tail or a whole round where no tail applies).  `short_tail` here is the
// model's own ESTIMATE of whether a tail applies, not short_tail_rows1's condition (no M % 256, no count of 96-row tiles, no look
// at the last segment).  The two are kept apart: merging them changes decisions.  ME_GEMM_TALL=0 turns it off.
inline bool tall_tile_wins(int64_t M, int64_t N, int64_t K, int seg1, int seg2, int C, const TileKnobs& knobs) {
    if (!knobs.tall || N % 256 || K < 128 || C < 256) return false;
    const int64_t nbn = N / 256;
    const int64_t tiles352 = (int64_t)seg_row_tiles<352>((int)M, seg1, seg2) * nbn;
    const int64_t tiles256 = cdiv(M, 256) * nbn;
    const double cost352 = (double)cdiv(tiles352, kRoundWorkgroups) * 352.0;
    const int64_t whole = tiles256 / kRoundWorkgroups, rem = tiles256 % kRoundWorkgroups;
    const bool short_tail = whole >= 1 && rem != 0 && 2 * rem <= kRoundWorkgroups && kRoundWorkgroups % nbn == 0;
    const double cost256 = ((double)whole + (rem == 0 ? 0.0 : (short_tail ? 0.69 : 1.0))) * 256.0;
    // a near-tie goes to the tall tile: qkv's 768 tall tiles (three exact rounds, 1056) against 1020 tiles of
    // 256 x 256 (3.98 rounds, 1024) measured 0.5 % faster in the step (23.27 -> 23.16 ms, three alternating runs)
    return cost352 * knobs.tall_bias < cost256;
}

// ... and its fp8 form (gemm_fp8.hip gemm_pp8t_kernel against gemm_pp8_kernel), without the short-tail form the fp8 path does not
// have.  A row of the tall tile costs about a tenth more there (weights one slab ahead instead of two), hence 1.1 where the 16-bit
// model has 0.95: fc1 at one image -- four rounds of 352 against six of 256, 1408 : 1536 -- measured 3.40 against 3.33 ms per step
// on the 256-row tile.  knob: ME_FP8_TALL, 0 turns it off, 1 forces it.
inline bool fp8_tall_wins(int64_t M, int64_t N, int seg1, int seg2, int knob) {
    if (knob == 0) return false;
    if (knob == 1) return true;
    const int64_t nbn = N / 256;
    const double cost352 = (double)cdiv((int64_t)seg_row_tiles<352>((int)M, seg1, seg2) * nbn, kRoundWorkgroups) * 352.0;
    const double cost256 = (double)cdiv(cdiv(M, 256) * nbn, kRoundWorkgroups) * 256.0;
    return cost352 * 1.1 < cost256;
}

// What one ViT linear over all row segments launches.  resid: the residual update x += gamma * (A W^T + b) (proj, fc2; N = C), else
// the 16-bit output form (qkv, fc1).  ln_wanted: the caller has a LayerNorm to put behind the update; ln_fusable: pipeline.hip
// ln_fusable()'s answer (it asks the occupancy API).  When the fused form applies it applies at EVERY batch size -- the tall tile is
// then taken whatever tall_tile_wins says --, so that a row's statistics are summed in the same order whatever batch the row is part of.
enum VitLinearKind {
    VIT_FUSED_LN_352,  // one launch on CFG_PP352 with the LayerNorm of the updated rows in its epilogue
    VIT_TALL_352,      // one launch on CFG_PP352
    VIT_ROUNDS_TAIL,   // rows1 rows on CFG_PP256 (whole rounds), the rest on CFG_PP96
    VIT_SINGLE         // one launch on cfg (-1: gemm_launch's automatic choice)
};
struct VitLinearPlan {
    VitLinearKind kind;
    int cfg;
    int64_t rows1;
};
inline VitLinearPlan vit_linear_plan(int64_t M, int64_t N, int64_t K, int seg1, int seg2, int C, bool resid, bool ln_wanted,
                                     bool ln_fusable, const TileKnobs& knobs) {
    if (!resid) {
        // fc1 at one image: five whole rounds + 224 short tiles instead of a sixth round a third full (qkv's 1020 tiles
        // are 3.98 rounds and N = 3072 does not divide the round: short_tail_rows1 declines)
        if (tall_tile_wins(M, N, K, seg1, seg2, C, knobs)) return {VIT_TALL_352, CFG_PP352, 0};
        if (C >= 256)
            if (const int64_t rows1 = short_tail_rows1(M, N, K, seg1, seg2, knobs)) return {VIT_ROUNDS_TAIL, CFG_PP256, rows1};
        return {VIT_SINGLE, -1, 0};
    }
    // the two-group 256x256 kernel (the cost model rates 128x128 a hair cheaper here; measured it is not).  Its
    // 192-row form (CFG_PP192; the segment order makes every boundary a multiple of 192 at one image)
    // wins for proj stand-alone (94.7 -> 80.3 us) and loses in the step (90 -> 95.6 us per launch, same box,
    // bench.py A/B): ME_GEMM_PP192=1 selects it for that comparison.
    const bool pp = C >= 256 && K >= 128;
    const bool pp192 = pp && K <= 1024 && knobs.pp192 && seg1 % 192 == 0 && seg2 % 192 == 0;
    if (ln_wanted && pp && ln_fusable) return {VIT_FUSED_LN_352, CFG_PP352, 0};
    if (pp && !pp192 && tall_tile_wins(M, N, K, seg1, seg2, C, knobs)) return {VIT_TALL_352, CFG_PP352, 0};
    if (pp && !pp192)
        if (const int64_t rows1 = short_tail_rows1(M, N, K, seg1, seg2, knobs)) return {VIT_ROUNDS_TAIL, CFG_PP256, rows1};
    return {VIT_SINGLE, pp192 ? CFG_PP192 : (pp ? CFG_PP256 : -1), 0};
}

// ---- split-K (pipeline.hip maybe_split_k) --------------------------------------------------
// Deterministic split-K for the small deep launches of the tail (gemm_core.h gemm_kernel<..., SPLITK>; VERDICT r4 "missing" 6): a
// launch whose image has fewer than 200 tiles of 128 x 128 and K >= ME_SPLIT_K_MINK (4096) runs on that tile with S work items per
// tile, S the largest power of two that keeps the launch within 640 work items and a K range of at least 512.  Decided from ONE
// image's rows, so a batch takes the decision of its images (a batch stays a loop of batch-one calls bit for bit).  OFF unless
// ME_SPLIT_K=1: measured, the two K = 9216 convolutions it applies to gain 0.02 ms per step together, and with a lower K bound (the
// 96 x 96 level's 3x3 convolutions, the upsample chains' 1x1) the partials' round trip through memory costs more than the longer K
// loop it replaces (+0.15 ms at K >= 2048).  Returns S; 1: no split.
inline int split_k_factor(int64_t rows_per_image, int64_t M, int64_t N, int64_t K, const TileKnobs& knobs) {
    if (!knobs.split_k || rows_per_image <= 0 || K < knobs.split_k_min_k) return 1;
    const int64_t tiles_img = cdiv(rows_per_image, 128) * cdiv(N, 128);
    if (tiles_img >= 200) return 1;
    int S = 1;
    while (S < 8 && tiles_img * (S * 2) <= 640 && K / (S * 2) >= 512) S *= 2;
    if (cdiv(M, 128) * cdiv(N, 128) > 4096) return 1;  // (the workspace's counters: pipeline.hip)
    return S;
}

}  // namespace me
