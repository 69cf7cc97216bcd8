// Slide-level survival probe on frozen features (gv_surv_train / gv_surv_predict / gv_cox_eval): the gated-attention ABMIL body
// of mil.hip with one risk output, trained on Cox's partial likelihood (Breslow ties, right-censoring).  Definitions: gipvit.h.
// The Cox loss couples the bags of a step (a bag's gradient depends on every other bag's risk), so the step is cut into four
// launches, every dependency a launch boundary (no grid barrier, no atomics):
//   mil_gate_kernel    unchanged (mil_common.h).
//   surv_pool_kernel   one workgroup per bag: scores, softmax, z (bag_softmax_pool, mil_common.h, as in mil_pool_kernel) and the
//                      risk theta_b = Wc . z + bc, this kernel's own middle.  With one output dz_b =
//                      dtheta_b Wc, so the backward down to the scores is linear in dtheta_b: the launch leaves the unit-gradient
//                      ds~_i = a_i (u_i - sum_j a_j u_j), u_i = Wc . x_i, and dbw~ = sum_i ds~_i (bag_score_grad on Wc).  Predict
//                      stops after theta.
//   surv_cox_kernel    one workgroup per bag, each from the step's <= 64 risks (O(m^2), the same arithmetic in every workgroup):
//                      M, S_i, its own dtheta_b and event term, then ds_i = dtheta_b ds~_i over the bag's rows and dbw_b.
//   mil_update_kernel  <SURV>: DL[b] = dtheta_b, the gradient of bc forced to zero, nothing at all in a step without an event.
// The entry points are the MIL probe's step driver (mil_common.h) with one more launch and the time / event / EV pointers.
// Sums run in step order (j, i), row order or over a fixed tree: results are bitwise the same run to run.
// gv_cox_eval: the cohort's partial likelihood in fp64 and the pair counts of Harrell's C, all pairs, a workgroup per row.
#include "mil_common.h"

namespace {

constexpr int STH = 1;        // column of a bag's DL row that carries theta_b from the pool launch to the Cox launch (column 0: dtheta_b)
constexpr int CMAXN = 65536;  // gv_cox_eval's largest cohort

// (b) one bag: softmax over its rows, z, the risk; training: the unit-gradient ds~ and dbw~
template <bool TRAIN>
__global__ __launch_bounds__(256) void surv_pool_kernel(MilP p) {
    __shared__ float sS[MMAXBAG];                                      // s_i, then exp(s_i - max), then a_i
    __shared__ float sU[TRAIN ? MMAXBAG : 1];                          // u_i = Wc . x_i
    __shared__ __attribute__((aligned(16))) float sZ[MMAXF];           // z, then Wc
    __shared__ __attribute__((aligned(16))) float zpart[4 * 256];
    __shared__ float red[256];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int F = p.F, L = p.L, b = blockIdx.x;
    int start, n, y;
    const bool ok = mil_bag(p, b, start, n, y);
    if (TRAIN && b == 0)                                               // the copy of w the update launch reads
        for (int l = t; l < L; l += 256) p.WS[l] = p.P[p.oB + 2 * L + l];
    if (!ok) {
        if (TRAIN) {
            if (t < MMAXC) p.DL[b * MMAXC + t] = 0.f;
            if (t == 0) { p.LOSS[b] = 0.f; p.DBW[b] = 0.f; }
        } else if (t == 0) {
            p.prob[p.off + b] = 0.f;
        }
        return;
    }
    bag_softmax_pool<TRAIN>(p, b, start, n, p.P[p.oB + 3 * L + 1], sS, sZ, zpart, red);
    // the risk: a lane's columns in order, then the wave's fixed tree (the MIL probe's logit at C = 1)
    const float* Wc = p.P + p.oWc;
    if (wave == 0) {
        float acc = 0.f;
        for (int f = lane; f < F; f += 64) acc = fmaf(Wc[f], sZ[f], acc);
        acc = wave_sum(acc);
        if (lane == 0) {
            const float theta = acc + p.P[p.oB + 3 * L];
            if (TRAIN) {
                p.DL[b * MMAXC] = 0.f;
                p.DL[b * MMAXC + STH] = theta;
            } else {
                p.prob[p.off + b] = theta;
            }
        }
    }
    if (!TRAIN) return;
    __syncthreads();
    for (int f = t; f < F; f += 256) sZ[f] = Wc[f];
    __syncthreads();
    bag_score_grad(p, b, start, n, sS, sU, sZ, red);              // u_i = Wc . x_i, then the unit-gradient ds~_i and dbw~
}

// (c) bag b of the step: Cox's dtheta_b and event term from the step's risks, then the bag's rows scaled
__global__ __launch_bounds__(256) void surv_cox_kernel(MilP p) {
    __shared__ float sT[MMAXBATCH], sTh[MMAXBATCH], sW[MMAXBATCH], sSum[MMAXBATCH];
    __shared__ int sE[MMAXBATCH];                                      // 1 / 0: event / censored, -1: a bad bag or no bag
    __shared__ float sOut[2];
    const int t = threadIdx.x, b = blockIdx.x;
    if (t < MMAXBATCH) {
        int s_, n_, y_;
        int e = -1;
        float tm = 0.f, th = 0.f;
        if (mil_bag(p, t, s_, n_, y_)) {                               // (a good bag: its index is inside the tables)
            const int bag = p.bags ? p.bags[p.off + t] : p.off + t;
            e = p.event[bag];
            tm = p.time[bag];
            th = p.DL[t * MMAXC + STH];
        }
        sE[t] = e; sT[t] = tm; sTh[t] = th;
    }
    __syncthreads();
    const int m = p.m;
    int ev = 0;
    float M = -INFINITY;
    for (int j = 0; j < m; ++j)
        if (sE[j] >= 0) { ev += sE[j]; M = fmaxf(M, sTh[j]); }
    if (ev == 0) {                                   // a step without an event: the update launch returns at once
        if (t == 0) {
            p.DL[b * MMAXC] = 0.f;
            p.LOSS[b] = 0.f;
            if (b == 0) p.EV[0] = 0.f;
        }
        return;
    }
    if (t < m) sW[t] = sE[t] >= 0 ? expf(sTh[t] - M) : 0.f;
    __syncthreads();
    if (t < m) {                                     // S_i, j in step order
        float s = 0.f;
        if (sE[t] >= 0)
            for (int j = 0; j < m; ++j)
                if (sE[j] >= 0 && sT[j] >= sT[t]) s += sW[j];
        sSum[t] = s;
    }
    __syncthreads();
    if (t == 0) {
        float dth = 0.f, term = 0.f;
        if (sE[b] >= 0) {
            float d = 0.f;
            for (int i = 0; i < m; ++i)              // i in step order
                if (sE[i] == 1 && sT[i] <= sT[b]) d += sW[b] / sSum[i];
            dth = (d - (float)sE[b]) / (float)ev;
            if (sE[b] == 1) term = logf(sSum[b]) - (sTh[b] - M);
        }
        p.DL[b * MMAXC] = dth;
        p.LOSS[b] = term;
        if (b == 0) p.EV[0] = (float)ev;
        sOut[0] = dth;
    }
    __syncthreads();
    if (sE[b] < 0) return;
    const float dth = sOut[0];
    int start, n, y;
    mil_bag(p, b, start, n, y);
    const long slot0 = (long)b * p.max_bag;
    for (int i = t; i < n; i += 256) p.DS[slot0 + i] *= dth;
    if (t == 0) p.DBW[b] *= dth;
}

__device__ __forceinline__ bool cox_valid(float th, float tm, int e) {
    return isfinite(th) && isfinite(tm) && tm >= 0.f && (e == 0 || e == 1);
}

struct CoxP {
    const float* risk; const float* time; const int* event;
    double* loss; long long* counts;
    double *W, *TERM, *HDR;       // workspace: exp(theta_j - M) or 0 | the rows' event terms | {M}
    long long* CNT;               // [n, 4]: the rows' comparable, concordant, discordant, tied
    int n;
};

// M over the valid entries, then W_j = exp(theta_j - M) (0 for an excluded entry)
__global__ __launch_bounds__(256) void cox_prep_kernel(CoxP p) {
    __shared__ float red[256];
    const int t = threadIdx.x;
    float mx = -INFINITY;
    for (int j = t; j < p.n; j += 256) {
        const float th = p.risk[j];
        if (cox_valid(th, p.time[j], p.event[j])) mx = fmaxf(mx, th);
    }
    mx = mil_block_max(mx, red, t);
    if (t == 0) p.HDR[0] = (double)mx;
    for (int j = t; j < p.n; j += 256) {
        const float th = p.risk[j];
        p.W[j] = cox_valid(th, p.time[j], p.event[j]) ? exp((double)th - (double)mx) : 0.0;
    }
}

// row i against every j: its risk-set sum (thread t the entries t, t + 256, .. in order, then one tree) and its pair counts
__global__ __launch_bounds__(256) void cox_row_kernel(CoxP p) {
    __shared__ double rs[256];
    __shared__ int rc[4][256];
    const int t = threadIdx.x, i = blockIdx.x;
    const float thi = p.risk[i], ti = p.time[i];
    const int ei = p.event[i];
    if (!cox_valid(thi, ti, ei) || ei == 0) {        // (uniform) only an event row has a term and comparable pairs
        if (t == 0) p.TERM[i] = 0.0;
        if (t < 4) p.CNT[(long)i * 4 + t] = 0;
        return;
    }
    double s = 0.0;
    int c[4] = {0, 0, 0, 0};
    for (int j = t; j < p.n; j += 256) {
        const float thj = p.risk[j], tj = p.time[j];
        if (!cox_valid(thj, tj, p.event[j])) continue;
        if (tj >= ti) s += p.W[j];
        if (ti < tj) {
            ++c[0];
            if (thi > thj) ++c[1];
            else if (thi < thj) ++c[2];
            else ++c[3];
        }
    }
    rs[t] = s;
#pragma unroll
    for (int k = 0; k < 4; ++k) rc[k][t] = c[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            rs[t] += rs[t + o];
#pragma unroll
            for (int k = 0; k < 4; ++k) rc[k][t] += rc[k][t + o];
        }
        __syncthreads();
    }
    if (t == 0) p.TERM[i] = log(rs[0]) - ((double)thi - p.HDR[0]);
    if (t < 4) p.CNT[(long)i * 4 + t] = rc[t][0];
}

// the rows' terms added in index order; the counts
__global__ __launch_bounds__(256) void cox_finish_kernel(CoxP p) {
    __shared__ double st[256];
    __shared__ long long rc[6][256];
    const int t = threadIdx.x;
    double total = 0.0;
    long long c[6] = {0, 0, 0, 0, 0, 0};             // events, comparable, concordant, discordant, tied, excluded
    for (int i0 = 0; i0 < p.n; i0 += 256) {
        const int i = i0 + t;
        __syncthreads();
        st[t] = i < p.n ? p.TERM[i] : 0.0;
        __syncthreads();
        if (t == 0) {
            const int k = p.n - i0 < 256 ? p.n - i0 : 256;
            for (int j = 0; j < k; ++j) total += st[j];
        }
        if (i < p.n) {
            const int e = p.event[i];
            if (cox_valid(p.risk[i], p.time[i], e)) c[0] += e;
            else ++c[5];
#pragma unroll
            for (int k = 0; k < 4; ++k) c[1 + k] += p.CNT[(long)i * 4 + k];
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) rc[k][t] = c[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int k = 0; k < 6; ++k) rc[k][t] += rc[k][t + o];
        }
        __syncthreads();
    }
    if (t == 0) p.loss[0] = total;
    if (t < 6) p.counts[t] = rc[t][0];
}

int cox_check_n(const char* who, int n) {
    GV_REQUIRE(n >= 1 && n <= CMAXN, GV_E_SHAPE, "%s: need 1 <= n <= %d (got %d)", who, CMAXN, n);
    return GV_OK;
}

// the MIL workspace at C = 1 and, behind it, the step's event count (4 floats keep the total a multiple of 16 bytes)
int64_t surv_workspace_floats(const MilWs& w) { return w.total + 4; }

}  // namespace

extern "C" int64_t gv_surv_workspace_bytes(int32_t batch, int32_t max_bag, int32_t L, int32_t F) {
    if (mil_check_shape("gv_surv_workspace_bytes", batch, max_bag, L, 1, F) != GV_OK) return -1;
    return surv_workspace_floats(mil_workspace(batch, max_bag, L, F)) * 4;
}

extern "C" int gv_surv_train(const gv_surv_train_args* a, void* stream) {
    const char* who = "gv_surv_train";
    GV_REQUIRE(a && a->params && a->m && a->v && a->x && a->bag_ptr && a->time && a->event && a->bags && a->loss_sum, GV_E_NULL,
               "%s: null pointer (params, m, v, x, bag_ptr, time, event, bags and loss_sum are required)", who);
    int rc = mil_check_shape(who, a->batch, a->max_bag, a->L, 1, a->F);
    if (rc != GV_OK) return rc;
    const MilWs w = mil_workspace(a->batch, a->max_bag, a->L, a->F);
    if ((rc = mil_check_common(who, "gv_surv_workspace_bytes", a->x, a->ldx, a->F, a->N, a->n_all_bags, a->n_bags, a->params, a->workspace,
                               a->workspace_bytes, surv_workspace_floats(w) * 4)) != GV_OK)
        return rc;
    if ((rc = mil_check_adam(who, a->m, a->v, a->step0, a->lr, a->lr_scale, a->wd, a->beta1, a->beta2, a->eps)) != GV_OK) return rc;
    MilP p = {};
    mil_fill(p, a->x, a->ldx, a->bag_ptr, nullptr, a->bags, a->N, a->F, a->L, 1, a->n_all_bags, a->max_bag, a->params, a->workspace, w);
    p.time = a->time; p.event = a->event; p.EV = (float*)a->workspace + w.total;
    p.Pm = a->m; p.Pv = a->v; p.loss = a->loss_sum;
    p.wd = a->wd; p.beta1 = a->beta1; p.beta2 = a->beta2; p.eps = a->eps;
    int64_t step = a->step0;
    mil_each_group(p, a->n_bags, a->batch, [&] {
        mil_set_step(p, a->lr, a->lr_scale, a->beta1, a->beta2, ++step);
        mil_launch_gate<true>(p, stream);
        hipLaunchKernelGGL(surv_pool_kernel<true>, dim3((unsigned)p.m), dim3(256), 0, (hipStream_t)stream, p);
        hipLaunchKernelGGL(surv_cox_kernel, dim3((unsigned)p.m), dim3(256), 0, (hipStream_t)stream, p);
        mil_launch_update<true>(p, stream);
    });
    GV_LAUNCH_CHECK(who);
    return GV_OK;
}

extern "C" int gv_surv_predict(const gv_surv_predict_args* a, void* stream) {
    const char* who = "gv_surv_predict";
    GV_REQUIRE(a && a->params && a->x && a->bag_ptr && a->risk, GV_E_NULL, "%s: null pointer (params, x, bag_ptr and risk are required)", who);
    const int M = mil_predict_group(a->n_bags);
    int rc = mil_check_shape(who, M, a->max_bag, a->L, 1, a->F);
    if (rc != GV_OK) return rc;
    const MilWs w = mil_workspace(M, a->max_bag, a->L, a->F);
    if ((rc = mil_check_common(who, "gv_surv_workspace_bytes", a->x, a->ldx, a->F, a->N, a->n_all_bags, a->n_bags, a->params, a->workspace,
                               a->workspace_bytes, surv_workspace_floats(w) * 4)) != GV_OK)
        return rc;
    MilP p = {};
    mil_fill(p, a->x, a->ldx, a->bag_ptr, nullptr, a->bags, a->N, a->F, a->L, 1, a->n_all_bags, a->max_bag, const_cast<float*>(a->params), a->workspace, w);
    p.prob = a->risk; p.attn = a->attn; p.score = a->score;
    mil_each_group(p, a->n_bags, M, [&] {
        mil_launch_gate<false>(p, stream);
        hipLaunchKernelGGL(surv_pool_kernel<false>, dim3((unsigned)p.m), dim3(256), 0, (hipStream_t)stream, p);
    });
    GV_LAUNCH_CHECK(who);
    return GV_OK;
}

// workspace, in 8-byte units: W [n] | TERM [n] | CNT [n, 4] | HDR [2]
extern "C" int64_t gv_cox_eval_workspace_bytes(int32_t n) {
    if (cox_check_n("gv_cox_eval_workspace_bytes", n) != GV_OK) return -1;
    return ((int64_t)6 * n + 2) * 8;
}

extern "C" int gv_cox_eval(const gv_cox_eval_args* a, void* stream) {
    const char* who = "gv_cox_eval";
    GV_REQUIRE(a && a->risk && a->time && a->event && a->loss && a->counts, GV_E_NULL,
               "%s: null pointer (risk, time, event, loss and counts are required)", who);
    int rc = cox_check_n(who, a->n);
    if (rc != GV_OK) return rc;
    const int64_t need = ((int64_t)6 * a->n + 2) * 8;
    GV_REQUIRE(a->workspace, GV_E_NULL, "%s: null workspace (%lld bytes needed, gv_cox_eval_workspace_bytes)", who, (long long)need);
    GV_REQUIRE(a->workspace_bytes >= need, GV_E_SHAPE, "%s: workspace of %lld bytes, %lld needed (gv_cox_eval_workspace_bytes)", who,
               (long long)a->workspace_bytes, (long long)need);
    GV_REQUIRE(gv_aligned(a->workspace, 8) && gv_aligned(a->loss, 8) && gv_aligned(a->counts, 8), GV_E_ALIGN,
               "%s: workspace, loss and counts must be 8-byte aligned", who);
    CoxP p = {};
    p.risk = a->risk; p.time = a->time; p.event = a->event; p.loss = a->loss; p.counts = (long long*)a->counts; p.n = a->n;
    p.W = (double*)a->workspace;
    p.TERM = p.W + a->n;
    p.CNT = (long long*)(p.TERM + a->n);
    p.HDR = (double*)(p.CNT + (int64_t)4 * a->n);
    hipLaunchKernelGGL(cox_prep_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(cox_row_kernel, dim3((unsigned)a->n), dim3(256), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(cox_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, p);
    GV_LAUNCH_CHECK(who);
    return GV_OK;
}
