// Attention-MIL probe on frozen features (gv_mil_train / gv_mil_predict): gated-attention ABMIL over bags of feature rows, one
// bag per slide, trained with Adam.  Model, step and parameter layout: include/gipvit.h.
// A step is three launches, every dependency a launch boundary (no grid barrier, no atomics).  What the survival probe
// (survival.hip) shares is in mil_common.h: the gate and update kernels, the pool kernel's front (bag_softmax_pool: scores,
// softmax, z) and back (bag_score_grad: da_i, ds_i, dbw), the checks and the step driver's pieces.  Here: the pool kernel's middle
// (logits, p, loss, dl, dz), predict's loss launch and the entry points.
//   mil_gate_kernel    grid (64-row tiles of a bag, bags of the step, 32-unit chunks of L): the [64, 32 | 32] pre-activations of
//                      V and U come off the f32 MFMA (v_mfma_f32_16x16x4_f32, the k-major LDS operand images and row stride of
//                      linprobe.hip); a lane holds t and g of the same (row, unit), so tanh, sigmoid and the chunk's share of the
//                      score w . (t * g) are lane-local plus one 16-lane sum.  t, g and the partial scores go to the workspace.
//   mil_pool_kernel    one workgroup per bag: scores (partials added in chunk order), softmax over the bag's own rows, z, logits,
//                      p, the loss, dl, dz, then da_i = dz . x_i and ds_i.  Predict stops after p.
//   mil_update_kernel  grid (32-column slices of F, 64-column blocks of the hidden axis [dt | dg | du]): dV | dU = (dt | dg)^T x
//                      over the step's rows, bags in step order and rows in order (a bag's last 64-row k step is zero-padded,
//                      which adds exact zeros); the (dt | dg) operand image is built on the fly from t, g, ds and w.  Adam runs
//                      in the epilogue.  The first slice's workgroups also sum their image's columns in row order: dbv, dbu and
//                      (from the du = ds t g columns, which take no part in the product) dw.  One more row of workgroups does
//                      dWc = sum_b dl_b z_b^T per slice, and its first also dbc, dbw and loss_sum over the bags in order.
// w is read by every update workgroup and stepped by one of them: the pool launch leaves a copy in the workspace for the readers.
// Every sum has an order fixed by the data layout (a fmaf chain in row order, a fixed tree over a workgroup's threads, chunk
// order, bag order), none depends on the grid: results are bitwise the same run to run.  Loads are bounds-checked by
// construction: a padded lane (row past the bag, k >= F, hidden column past its range) is zero-filled in both operands, never
// read.  A bad bag (gipvit.h) is recognised by every kernel from bag_ptr / labels alone and is never used as an index.
#include "mil_common.h"

namespace {

// (b) one bag: softmax over its rows, z, logits, p, loss; training: dl, dz, da, ds
template <bool TRAIN>
__global__ __launch_bounds__(256) void mil_pool_kernel(MilP p) {
    __shared__ float sS[MMAXBAG];                                      // s_i, then exp(s_i - max), then a_i
    __shared__ float sDA[TRAIN ? MMAXBAG : 1];
    __shared__ __attribute__((aligned(16))) float sZ[MMAXF];           // z, then dz
    __shared__ __attribute__((aligned(16))) float zpart[4 * 256];
    __shared__ float red[256];
    __shared__ float sLg[MMAXC], sDL[MMAXC];
    __shared__ int sflag[MMAXBATCH];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int F = p.F, L = p.L, C = p.C, b = blockIdx.x;
    int start, n, y;
    const bool ok = mil_bag(p, b, start, n, y);
    float inv_m = 0.f;
    if (TRAIN) {
        if (t < MMAXBATCH) { int s_, n_, y_; sflag[t] = mil_bag(p, t, s_, n_, y_) ? 1 : 0; }
        __syncthreads();
        int good = 0;
        for (int j = 0; j < MMAXBATCH; ++j) good += sflag[j];
        inv_m = good > 0 ? 1.f / (float)good : 0.f;
        if (b == 0)                                                    // the copy of w the update launch reads
            for (int l = t; l < L; l += 256) p.WS[l] = p.P[p.oB + 2 * L + l];
    }
    if (!ok) {
        if (TRAIN) {
            if (t < MMAXC) p.DL[b * MMAXC + t] = 0.f;
            if (t == 0) { p.LOSS[b] = 0.f; p.DBW[b] = 0.f; }
        } else {
            if (t < C) p.prob[(long)(p.off + b) * C + t] = 0.f;
            if (t == 0) p.LOSS[b] = 0.f;
        }
        return;
    }
    bag_softmax_pool<TRAIN>(p, b, start, n, p.P[p.oB + 3 * L + C], sS, sZ, zpart, red);
    // logits: a wave per class, a lane's columns in order, then the wave's fixed tree
    const float* Wc = p.P + p.oWc;
    for (int c = wave; c < C; c += 4) {
        float acc = 0.f;
        for (int f = lane; f < F; f += 64) acc = fmaf(Wc[(long)c * F + f], sZ[f], acc);
        acc = wave_sum(acc);
        if (lane == 0) sLg[c] = acc + p.P[p.oB + 3 * L + c];
    }
    __syncthreads();
    if (t == 0) {
        float zm = sLg[0];
        for (int c = 1; c < C; ++c) zm = fmaxf(zm, sLg[c]);
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += expf(sLg[c] - zm);
        p.LOSS[b] = y >= 0 ? logf(s) - (sLg[y] - zm) : 0.f;
        for (int c = 0; c < C; ++c) {
            const float pc = expf(sLg[c] - zm) / s;
            if (TRAIN) {
                const float d = (pc - (c == y ? 1.f : 0.f)) * inv_m;
                sDL[c] = d;
                p.DL[b * MMAXC + c] = d;
            } else {
                p.prob[(long)(p.off + b) * C + c] = pc;
            }
        }
    }
    if (!TRAIN) return;
    __syncthreads();
    for (int f = t; f < F; f += 256) {               // dz = Wc^T dl, classes in order
        float d = 0.f;
        for (int c = 0; c < C; ++c) d = fmaf(Wc[(long)c * F + f], sDL[c], d);
        sZ[f] = d;
    }
    __syncthreads();
    bag_score_grad(p, b, start, n, sS, sDA, sZ, red);             // da_i = dz . x_i, then ds_i and dbw
}

// predict's loss: the group's bag losses added one by one, so that a list split over two calls gives the same bits
__global__ __launch_bounds__(64) void mil_loss_kernel(MilP p) {
    if (threadIdx.x != 0) return;
    float s = p.accumulate ? p.loss[0] : 0.f;
    for (int b = 0; b < p.m; ++b) s += p.LOSS[b];
    p.loss[0] = s;
}

}  // namespace

extern "C" int64_t gv_mil_workspace_bytes(int32_t batch, int32_t max_bag, int32_t L, int32_t C, int32_t F) {
    if (mil_check_shape("gv_mil_workspace_bytes", batch, max_bag, L, C, F) != GV_OK) return -1;
    return mil_workspace(batch, max_bag, L, F).total * 4;
}

extern "C" int gv_mil_train(const gv_mil_train_args* a, void* stream) {
    const char* who = "gv_mil_train";
    GV_REQUIRE(a && a->params && a->m && a->v && a->x && a->bag_ptr && a->labels && a->bags && a->loss_sum, GV_E_NULL,
               "%s: null pointer (params, m, v, x, bag_ptr, labels, bags and loss_sum are required)", who);
    int rc = mil_check_shape(who, a->batch, a->max_bag, a->L, a->C, a->F);
    if (rc != GV_OK) return rc;
    const MilWs w = mil_workspace(a->batch, a->max_bag, a->L, a->F);
    if ((rc = mil_check_common(who, "gv_mil_workspace_bytes", a->x, a->ldx, a->F, a->N, a->n_all_bags, a->n_bags, a->params, a->workspace,
                               a->workspace_bytes, w.total * 4)) != GV_OK)
        return rc;
    if ((rc = mil_check_adam(who, a->m, a->v, a->step0, a->lr, a->lr_scale, a->wd, a->beta1, a->beta2, a->eps)) != GV_OK) return rc;
    MilP p = {};
    mil_fill(p, a->x, a->ldx, a->bag_ptr, a->labels, a->bags, a->N, a->F, a->L, a->C, a->n_all_bags, a->max_bag, a->params, a->workspace, w);
    p.Pm = a->m; p.Pv = a->v; p.loss = a->loss_sum; p.need_label = 1;
    p.wd = a->wd; p.beta1 = a->beta1; p.beta2 = a->beta2; p.eps = a->eps;
    int64_t step = a->step0;
    mil_each_group(p, a->n_bags, a->batch, [&] {
        mil_set_step(p, a->lr, a->lr_scale, a->beta1, a->beta2, ++step);
        mil_launch_gate<true>(p, stream);
        hipLaunchKernelGGL(mil_pool_kernel<true>, dim3((unsigned)p.m), dim3(256), 0, (hipStream_t)stream, p);
        mil_launch_update<false>(p, stream);
    });
    GV_LAUNCH_CHECK(who);
    return GV_OK;
}

extern "C" int gv_mil_predict(const gv_mil_predict_args* a, void* stream) {
    const char* who = "gv_mil_predict";
    GV_REQUIRE(a && a->params && a->x && a->bag_ptr && a->prob, GV_E_NULL, "%s: null pointer (params, x, bag_ptr and prob are required)", who);
    GV_REQUIRE(!a->loss || a->labels, GV_E_NULL, "%s: null labels with a loss output (the loss is the sum of -log p[label])", who);
    const int M = mil_predict_group(a->n_bags);
    int rc = mil_check_shape(who, M, a->max_bag, a->L, a->C, a->F);
    if (rc != GV_OK) return rc;
    const MilWs w = mil_workspace(M, a->max_bag, a->L, a->F);
    if ((rc = mil_check_common(who, "gv_mil_workspace_bytes", a->x, a->ldx, a->F, a->N, a->n_all_bags, a->n_bags, a->params, a->workspace,
                               a->workspace_bytes, w.total * 4)) != GV_OK)
        return rc;
    MilP p = {};
    mil_fill(p, a->x, a->ldx, a->bag_ptr, a->loss ? a->labels : nullptr, a->bags, a->N, a->F, a->L, a->C, a->n_all_bags, a->max_bag,
             const_cast<float*>(a->params), a->workspace, w);
    p.prob = a->prob; p.loss = a->loss; p.attn = a->attn; p.score = a->score;
    mil_each_group(p, a->n_bags, M, [&] {
        p.accumulate = (p.off > 0 || a->accumulate) ? 1 : 0;
        mil_launch_gate<false>(p, stream);
        hipLaunchKernelGGL(mil_pool_kernel<false>, dim3((unsigned)p.m), dim3(256), 0, (hipStream_t)stream, p);
        if (a->loss) hipLaunchKernelGGL(mil_loss_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p);
    });
    GV_LAUNCH_CHECK(who);
    return GV_OK;
}
