// Stand-alone host program over csrc/attn_plan.h (plain g++, no HIP): reads the case lines tests/test_attn_plan_host.py writes from
// tests/traces/attention_plans.json and prints one line of integers per case, in the field order of the fixture's rows.
//   C                     the per-class tables: "fwd_cfg nkt nw pairs lds occ" and "bwd_cfg nkt kt nw pairs lds occ" per class
//   F N pairs             -> nkt grid block lds            B N pairs            -> nkt kt grid block lds
//   P N pairs q_rows      -> row? nkt grid block lds       S N pairs q_limit    -> query_blocks grid block lds
//   V pairs n N0 N1 [N2]  -> long segment (-1: one launch per segment) and, if fused, grid long_blocks block lds
#include "../gipmed-project-self-supervised-vit_amd/csrc/attn_plan.h"
#include <stdio.h>

using namespace gvattn;

template <int... C> static void print_cfgs(std::integer_sequence<int, C...>) {
    (printf("fwd_cfg %d %d %d %d %d\n", C, FwdCfg<C>::NW, FwdCfg<C>::PAIRS, FwdCfg<C>::LDS, FwdCfg<C>::OCC), ...);
    (printf("bwd_cfg %d %d %d %d %d %d\n", C, bwd_kt(C), BwdOf<C>::NW, BwdOf<C>::PAIRS, BwdOf<C>::LDS, BwdOf<C>::OCC), ...);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: attn_plan_main <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char buf[256];
    while (fgets(buf, sizeof(buf), f)) {
        int N = 0, pairs = 0, x = 0;
        const int got = sscanf(buf + 1, "%d %d %d", &N, &pairs, &x);
        if (buf[0] == 'C') {
            print_cfgs(Classes{});
        } else if (buf[0] == 'F' && got == 2) {
            const Launch l = with_class(N, [&](auto c) { return fwd_launch<decltype(c)::value>(pairs); });
            printf("%d %ld %d %d\n", class_of(N), l.grid, l.block, l.lds_bytes);
        } else if (buf[0] == 'B' && got == 2) {
            const Launch l = with_class(N, [&](auto c) { return bwd_launch<decltype(c)::value>(pairs); });
            printf("%d %d %ld %d %d\n", class_of(N), bwd_kt(class_of(N)), l.grid, l.block, l.lds_bytes);
        } else if (buf[0] == 'P' && got == 3) {
            const Launch l = with_class(N, [&](auto c) { return probs_launch<decltype(c)::value>(pairs, x); });
            printf("%d %d %ld %d %d\n", (int)probs_by_row(x), class_of(N), l.grid, l.block, l.lds_bytes);
        } else if (buf[0] == 'S' && got == 3) {
            const Launch l = StreamCfg::launch(pairs, 1, N, x);
            printf("%d %ld %d %d\n", StreamCfg::query_blocks(N, x), l.grid, l.block, l.lds_bytes);
        } else if (buf[0] == 'V') {
            int n = 0, Ns[3] = {0, 0, 0};
            if (sscanf(buf + 1, "%d %d %d %d %d", &pairs, &n, &Ns[0], &Ns[1], &Ns[2]) != 2 + n || n < 2 || n > 3) return 3;
            const int il = n == 2 ? varlen_long_segment(Ns[0], Ns[1]) : -1;      // as gv_attention_fwd_varlen asks
            const Launch l = VarlenCfg::launch(pairs, pairs);
            if (il < 0) printf("-1\n");
            else printf("%d %ld %d %d %d\n", il, l.grid, VarlenCfg::long_blocks(pairs), l.block, l.lds_bytes);
        } else {
            fprintf(stderr, "bad case line: %s", buf);
            return 3;
        }
    }
    fclose(f);
    return 0;
}
