// Stand-alone host program over ProbsStreamCfg of csrc/attn_plan.h (plain g++, no HIP), for tests/test_attention_probs_stream_host.py.
// First line: "cfg row_threads row_nw row_ch threads qb kb lds occ".  Then, per argument triple "n_img H q_rows" of the command line:
//   row? grid block lds query_blocks
#include "../gipmed-project-self-supervised-vit_amd/csrc/attn_plan.h"
#include <stdio.h>
#include <stdlib.h>

using C = gvattn::ProbsStreamCfg;

int main(int argc, char** argv) {
    if (argc < 4 || (argc - 1) % 3) { fprintf(stderr, "usage: attn_probs_stream_plan_main (n_img H q_rows)...\n"); return 2; }
    printf("cfg %d %d %d %d %d %d %d %d\n", C::ROW_THREADS, C::ROW_NW, C::ROW_CH, C::THREADS, C::QB, C::KB, C::LDS, C::OCC);
    for (int i = 1; i + 2 < argc; i += 3) {
        const int n_img = atoi(argv[i]), H = atoi(argv[i + 1]), q_rows = atoi(argv[i + 2]);
        const gvattn::Launch l = C::launch(n_img, H, q_rows);
        printf("%d %ld %d %d %d\n", (int)C::by_row(q_rows), l.grid, l.block, l.lds_bytes, C::query_blocks(q_rows));
    }
    return 0;
}
