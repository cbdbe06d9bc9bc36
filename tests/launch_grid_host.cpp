// Host driver of csrc/launch_grid.h for tests/test_launch_grid_cpu.py: the header and nothing else of the library.
// Reads one case per line from stdin and prints one result per line:
//   r <per_cu> <cus> <cu_granted>                   -> resident_workgroups
//   g <ntiles> <resident> <unit> <limit> <cap>      -> persistent_grid (-1: the LayerNorm round does not fit)
#include <cstdio>

#include "../matrix-eyes_amd/csrc/launch_grid.h"

int main() {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'r') {
            int per_cu, cus, granted;
            if (scanf("%d %d %d", &per_cu, &cus, &granted) != 3) return 2;
            printf("%d\n", me::resident_workgroups(per_cu, cus, granted));
        } else if (kind == 'g') {
            long long ntiles, unit;
            int resident, limit, cap;
            if (scanf("%lld %d %lld %d %d", &ntiles, &resident, &unit, &limit, &cap) != 5) return 2;
            printf("%lld\n", (long long)me::persistent_grid(ntiles, resident, unit, limit, cap));
        } else {
            return 2;
        }
    }
    return 0;
}
