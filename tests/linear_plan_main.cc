// Stand-alone host program over csrc/linear_plan.h (plain g++, no HIP): reads the case lines tests/linear_plan_cases.py writes from
// tests/traces/linear_plans.json and prints, per CU budget and case, "<budget>\t<kernel name>\t<scratch bytes>".  The name is the
// plan of the call as the row makes it (with or without a workspace); the bytes are the plan with the full scratch offered, which is
// what gv_workspace_bytes answers.
#include "../gipmed-project-self-supervised-vit_amd/csrc/linear_plan.h"
#include <string.h>
#include <string>
#include <vector>

using namespace gvplan;

static void* const P0 = (void*)(uintptr_t)(1 << 20);
static void* const P1 = (void*)(uintptr_t)(2 << 20);

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: linear_plan_main <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<std::string> lines;
    char buf[512];
    while (fgets(buf, sizeof(buf), f)) lines.push_back(buf);
    fclose(f);
    for (int budget : {256, 248}) {
        for (const std::string& line : lines) {
            const char* s = line.c_str();
            char name[96] = "";
            long long bytes = -1;
            if (s[0] == 'L') {
                int M, N, K, ta, tb, c_f32, epi, colsum_a, in_place, ws;
                if (sscanf(s + 1, "%d %d %d %d %d %d %d %d %d %d", &M, &N, &K, &ta, &tb, &c_f32, &epi, &colsum_a, &in_place, &ws) != 10) return 3;
                gv_linear_args a;
                memset(&a, 0, sizeof(a));
                a.A = P0; a.B = P0; a.C = P0; a.M = M; a.N = N; a.K = K;
                a.lda = ta ? M : K; a.ldb = tb ? N : K; a.ldc = a.ldr = a.ld_aux = N;
                a.trans_a = ta; a.trans_b = tb; a.c_is_f32 = c_f32; a.epilogue = epi; a.alpha = 1.f;
                if (epi & GV_EPI_BIAS) a.bias = (const float*)P0;
                if (epi & GV_EPI_RESID) a.resid = (const float*)(in_place ? a.C : P1);
                if (epi & GV_EPI_DGELU) a.aux_in = P0;
                if (epi & GV_EPI_SAVE_PRE) a.aux_out = P0;
                if (colsum_a) a.colsum_a = (float*)P0;
                gv_linear_args offered = a;
                offered.workspace = (float*)P0; offered.workspace_bytes = WORKSPACE_BYTES;
                if (ws) a = offered;
                linear_kernel_name(plan_linear(a, budget), a, name, sizeof(name));
                bytes = plan_linear(offered, budget).slab_bytes;
            } else if (s[0] == 'G') {
                gv_linear_dw_group_args a;
                memset(&a, 0, sizeof(a));
                int T, n, used = 0;
                if (sscanf(s + 1, "%d %d%n", &T, &n, &used) != 2 || n < 1 || n > GV_DW_GROUP_MAX) return 3;
                const char* p = s + 1 + used;
                for (int q = 0; q < n; ++q) {
                    int m, nn, u = 0;
                    if (sscanf(p, "%d %d%n", &m, &nn, &u) != 2) return 3;
                    p += u;
                    a.prob[q].M = m; a.prob[q].N = nn; a.prob[q].ldy = m; a.prob[q].ldx = nn; a.prob[q].ldw = nn;
                    a.prob[q].dY = P0; a.prob[q].X = P0; a.prob[q].dW = (float*)P0;
                }
                a.n = n; a.K = T; a.workspace = (float*)P0; a.workspace_bytes = WORKSPACE_BYTES;
                const DwGroupPlan pl = plan_dw_group(a, budget);
                snprintf(name, sizeof(name), "%s", group_kernel_name(pl));
                bytes = pl.slab_bytes;
            } else if (s[0] == 'F') {
                int op, M, K;
                if (sscanf(s + 1, "%d %d %d", &op, &M, &K) != 3) return 3;
                if (op == 2) panel_kernel_name(name, sizeof(name), pick_fm_mlp(M, budget), false, MODE_FWD, EP_MLP, false);
                else panel_kernel_name(name, sizeof(name), pick_fm(M, budget), op == 1, op == 1 ? MODE_BWD : MODE_FWD, 0, panel_pingpong(K));
            } else {
                continue;
            }
            printf("%d\t%s\t%lld\n", budget, name, bytes);
        }
    }
    return 0;
}
