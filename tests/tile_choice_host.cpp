// Host driver of csrc/tile_choice.h for tests/test_tile_choice_cpu.py: the header and nothing else of the library.
// Reads one case per line from stdin and prints one answer per line (tests/tile_choice_cases.py writes the lines):
//   n <id>                                                           -> name rows cols seg_align two_slab admits(hex) cf_modes
//   r <force> <M> <N> <K> <seg1> <seg2> <amode> <epi> <KH> <KW> <stride> <out_H> <out_W> <Cin> <tap_bias> <ln_out16>
//     <dynamic> <halo> <halo12> <halo128>                            -> "ok <cfg>" | "shape" | "arg"   (resolve_config + config_refusal)
//   v <M> <N> <K> <seg1> <seg2> <C> <resid> <ln_wanted> <ln_fusable>
//     <tall> <tall_bias> <tail96> <pp192>                            -> "lnf" | "tall" | "tail <rows1>" | "single <cfg>"
//   s <rows_per_image> <M> <N> <K> <on> <min_k>                      -> S
//   f <M> <N> <seg1> <seg2> <knob>                                   -> 0 | 1
#include <cstdio>

#include "../matrix-eyes_amd/csrc/tile_choice.h"

using namespace me;

int main() {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'n') {
            int id;
            if (scanf("%d", &id) != 1 || id < 0 || id >= CFG_COUNT) return 2;
            const TileConfig& c = kTileConfigs[id];
            printf("%s %d %d %d %d %x %d\n", c.name, c.rows, c.cols, c.seg_align, (int)c.two_slab, c.admits, (int)c.cf_modes);
        } else if (kind == 'r') {
            int force, tap, ln, dyn, halo, halo12, halo128;
            TileProblem q;
            if (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &force, &q.M, &q.N, &q.K, &q.seg1, &q.seg2, &q.amode, &q.epi,
                      &q.KH, &q.KW, &q.stride, &q.out_H, &q.out_W, &q.Cin, &tap, &ln, &dyn, &halo, &halo12, &halo128) != 20)
                return 2;
            q.tap_bias = tap != 0, q.ln_out16 = ln != 0;
            TileKnobs k;
            k.dynamic_tiles = dyn != 0, k.conv_halo = halo != 0, k.conv_halo12 = halo12 != 0, k.conv_halo128 = halo128 != 0;
            const int cfg = resolve_config(q, force, k);
            const TileRefusal r = config_refusal(q, cfg);
            if (r.kind == TILE_OK) printf("ok %d\n", cfg);
            else printf(r.kind == TILE_BAD_SHAPE ? "shape\n" : "arg\n");
        } else if (kind == 'v') {
            long long M, N, K;
            int seg1, seg2, C, resid, lnw, lnf, tall, tail96, pp192;
            double bias;
            if (scanf("%lld %lld %lld %d %d %d %d %d %d %d %lf %d %d", &M, &N, &K, &seg1, &seg2, &C, &resid, &lnw, &lnf, &tall, &bias, &tail96,
                      &pp192) != 13)
                return 2;
            TileKnobs k;
            k.tall = tall != 0, k.tall_bias = bias, k.tail96 = tail96 != 0, k.pp192 = pp192 != 0;
            const VitLinearPlan p = vit_linear_plan(M, N, K, seg1, seg2, C, resid != 0, lnw != 0, lnf != 0, k);
            if (p.kind == VIT_FUSED_LN_352) printf("lnf\n");
            else if (p.kind == VIT_TALL_352) printf("tall\n");
            else if (p.kind == VIT_ROUNDS_TAIL) printf("tail %lld\n", (long long)p.rows1);
            else printf("single %d\n", p.cfg);
        } else if (kind == 's') {
            long long rpi, M, N, K;
            int on, min_k;
            if (scanf("%lld %lld %lld %lld %d %d", &rpi, &M, &N, &K, &on, &min_k) != 6) return 2;
            TileKnobs k;
            k.split_k = on != 0, k.split_k_min_k = min_k;
            printf("%d\n", split_k_factor(rpi, M, N, K, k));
        } else if (kind == 'f') {
            long long M, N;
            int seg1, seg2, knob;
            if (scanf("%lld %lld %d %d %d", &M, &N, &seg1, &seg2, &knob) != 5) return 2;
            printf("%d\n", (int)fp8_tall_wins(M, N, seg1, seg2, knob));
        } else {
            return 2;
        }
    }
    return 0;
}
