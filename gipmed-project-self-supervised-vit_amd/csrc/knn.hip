// Weighted k-NN vote on frozen features (gv_knn_vote): DINO's knn_classifier as the training monitor of a --dino run.
//   sim = q . bank^T (f32, rows already L2-normalised), the k largest per query over the whole bank,
//   votes[q, c] = sum over those k of exp(sim * inv_temp) * [labels[idx] == c].
// The Q x Nb similarity matrix never leaves the chip: a workgroup owns 128 queries and one split of the bank, walks the split in
// 128-row chunks through the f32 MFMA tile of f32path.hip's Linear (128 x 128, four waves of 64 x 64, v_mfma_f32_16x16x4_f32,
// k-major LDS operand images, row stride 144), parks each chunk's similarity tile in LDS and lets one thread per query row scan
// it against the row's current k-th best, inserting survivors into a sorted (sim, idx) list of length k, also in LDS.  A second
// small kernel merges the n_split lists of a query and computes the votes.  No atomics: the result is the same run to run.
//
// Order (part of the contract): similarity descending, among equal similarities the smaller bank index first.  A split sees its
// rows in ascending index order and an equal newcomer never passes a resident, the merge compares (sim, idx) -- so the rule
// holds for every split count.  A similarity is one k-ordered fmaf chain whatever tile position it is computed at, so top_sim
// is bitwise the same for every split count too.
#include "gv_common.h"
#include <math.h>
#include <limits.h>

namespace {

constexpr int KQT = 128, KBT = 128, KBK = 16, KLD = 144;      // query tile, bank chunk, k step, operand image row stride
constexpr int KSLD = KBT + 1;                                   // similarity tile row stride: lane = row reads hit 64 banks
constexpr int KMAXK = 64, KMAXC = 32, KMAXD = 1024, KMAXSPLIT = 32;
constexpr int KOPER = 2 * KBK * KLD, KTILE = KQT * KSLD;        // floats

static inline int knn_lds_bytes(int k) { return (KOPER + KTILE + 2 * k * KQT) * 4; }

struct KnnP {
    gv_knn_vote_args a;
    int n_split, per;         // rows of the bank per split: split s owns [s * per, min(Nb, (s + 1) * per))
    float* ws_sim;            // [n_split, Q, k]
    int* ws_idx;              // [n_split, Q, k]
};

// one [128 rows x 16 k] tile of a row-major matrix, rows >= R and k >= K zero-filled (K and ld are multiples of 4, base 16-byte aligned)
__device__ __forceinline__ void knn_tile_load(const float* __restrict__ X, long ld, int r0, int R, int k0, int K, f32x4 (&v)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int idx = threadIdx.x + 256 * j, r = r0 + (idx >> 2), k = k0 + (idx & 3) * 4;
        v[j] = (r < R && k < K) ? *(const f32x4*)(X + (long)r * ld + k) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
__device__ __forceinline__ void knn_tile_store(float* S, const f32x4 (&v)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int idx = threadIdx.x + 256 * j, r = idx >> 2, k = (idx & 3) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) S[(k + i) * KLD + r] = v[j][i];
    }
}

// s beats the row's k-th best: residents smaller than s move one down, s takes the slot that frees.  An equal resident stays ahead
// (it has the smaller bank index).  Fixed trip count (k - 1), no early exit, no barrier.  Returns the new k-th best.
__device__ __forceinline__ float knn_insert(float* Lsim, int* Lidx, int t, int k, float s, int bi) {
    bool placed = false;
    float last = s;
#pragma unroll 4
    for (int j = k - 1; j >= 1; --j) {
        const float ps = Lsim[(j - 1) * KQT + t];
        const int pi = Lidx[(j - 1) * KQT + t];
        const bool mv = ps < s;
        if (mv || !placed) { Lsim[j * KQT + t] = mv ? ps : s; Lidx[j * KQT + t] = mv ? pi : bi; }
        if (j == k - 1) last = mv ? ps : s;
        placed = placed || !mv;
    }
    if (!placed) { Lsim[t] = s; Lidx[t] = bi; }
    return last;
}

__global__ __launch_bounds__(256) void knn_scan_kernel(KnnP p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const gv_knn_vote_args& a = p.a;
    float* As = sm;
    float* Bs = As + KBK * KLD;
    float* St = sm + KOPER;                        // [128][129] similarity tile of the current chunk
    float* Lsim = St + KTILE;                      // [k][128]: entry j of query row t at j * 128 + t (lane = row: no bank conflict)
    int* Lidx = (int*)(Lsim + a.k * KQT);
    const int Q = a.Q, D = a.D, k = a.k;
    const int q0 = blockIdx.x * KQT;
    const int b_lo = blockIdx.y * p.per, b_hi = min(a.Nb, b_lo + p.per);      // may be empty (b_lo >= Nb): the lists stay fillers
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, wm = wave >> 1, wn = wave & 1, li = lane & 15, g = lane >> 4;
    const int t = threadIdx.x;
    if (t < KQT)
        for (int j = 0; j < k; ++j) { Lsim[j * KQT + t] = -INFINITY; Lidx[j * KQT + t] = INT_MAX; }
    float thr = -INFINITY;                         // the row's current k-th best (rows t < 128 only)
    f32x4 ra[2], rb[2];
    if (b_lo < b_hi) {
        knn_tile_load(a.q, a.ldq, q0, Q, 0, D, ra);
        knn_tile_load(a.bank, a.ldb, b_lo, b_hi, 0, D, rb);
    }
    for (int b0 = b_lo; b0 < b_hi; b0 += KBT) {
        f32x4 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < D; k0 += KBK) {
            __syncthreads();                       // the previous step's fragment reads are done
            knn_tile_store(As, ra);
            knn_tile_store(Bs, rb);
            __syncthreads();
            if (k0 + KBK < D) {                    // next tile's loads fly under this tile's MFMAs
                knn_tile_load(a.q, a.ldq, q0, Q, k0 + KBK, D, ra);
                knn_tile_load(a.bank, a.ldb, b0, b_hi, k0 + KBK, D, rb);
            } else if (b0 + KBT < b_hi) {          // ... the next chunk's first tile under the scan
                knn_tile_load(a.q, a.ldq, q0, Q, 0, D, ra);
                knn_tile_load(a.bank, a.ldb, b0 + KBT, b_hi, 0, D, rb);
            }
#pragma unroll
            for (int kk = 0; kk < KBK / 4; ++kk) {
                float af[4], bf[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) af[i] = As[(kk * 4 + g) * KLD + wm * 64 + i * 16 + li];
#pragma unroll
                for (int j = 0; j < 4; ++j) bf[j] = Bs[(kk * 4 + g) * KLD + wn * 64 + j * 16 + li];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
        }
        // park the tile (accumulator fragment: row 4g + r, column li); the previous chunk's scan ended before this chunk's first barrier
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) St[(wm * 64 + i * 16 + g * 4 + r) * KSLD + wn * 64 + j * 16 + li] = acc[i][j][r];
        __syncthreads();
        if (t < KQT && q0 + t < Q) {
            const int ncol = min(KBT, b_hi - b0);  // padded bank rows are never looked at
            const float* row = St + t * KSLD;
            // 16 similarities at a time: the reads fly together and the common case (nothing beats the k-th best) is 16 compares;
            // candidates are then taken in column order against the threshold as it rises
            for (int c0 = 0; c0 < ncol; c0 += 16) {
                float sv[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) sv[i] = row[c0 + i];          // (columns >= ncol of the tile are in bounds; masked below)
                unsigned m = 0;
#pragma unroll
                for (int i = 0; i < 16; ++i) m |= (sv[i] > thr) ? (1u << i) : 0u;
                if (ncol - c0 < 16) m &= (1u << (ncol - c0)) - 1u;
                while (m) {
                    const int c = c0 + __ffs(m) - 1;
                    m &= m - 1;
                    const float s = row[c];
                    if (s > thr) thr = knn_insert(Lsim, Lidx, t, k, s, b0 + c);
                }
            }
        }
    }
    if (t < KQT && q0 + t < Q) {
        const long o = ((long)blockIdx.y * Q + q0 + t) * k;
        for (int j = 0; j < k; ++j) { p.ws_sim[o + j] = Lsim[j * KQT + t]; p.ws_idx[o + j] = Lidx[j * KQT + t]; }
    }
}

// One workgroup per query: every candidate of the n_split lists finds its rank in the merged order by binary search in the other
// lists (each is sorted in that order), ranks < k are the result; then one thread per class adds the votes in rank order.
__global__ __launch_bounds__(256) void knn_merge_kernel(KnnP p) {
    __shared__ float cs[KMAXSPLIT * KMAXK];
    __shared__ int ci[KMAXSPLIT * KMAXK];
    __shared__ float os[KMAXK];
    __shared__ int oi[KMAXK];
    const gv_knn_vote_args& a = p.a;
    const int q = blockIdx.x, k = a.k, n = p.n_split * k, Q = a.Q;
    for (int e = threadIdx.x; e < n; e += 256) {
        const int s = e / k, j = e - s * k;
        const long o = ((long)s * Q + q) * k + j;
        cs[e] = p.ws_sim[o];
        ci[e] = p.ws_idx[o];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += 256) {
        const int s = e / k;
        const float ms = cs[e];
        const int mi = ci[e];
        int rank = e - s * k;
        for (int s2 = 0; s2 < p.n_split; ++s2) {
            if (s2 == s) continue;
            int lo = 0, hi = k;                    // how many of list s2 rank ahead of this candidate
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const float xs = cs[s2 * k + mid];
                const int xi = ci[s2 * k + mid];
                const bool ahead = xs > ms || (xs == ms && (xi < mi || (xi == mi && s2 < s)));
                if (ahead) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        if (rank < k) { os[rank] = ms; oi[rank] = mi; }
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < k) {
        if (a.top_sim) a.top_sim[(long)q * k + c] = os[c];
        if (a.top_idx) a.top_idx[(long)q * k + c] = oi[c];
    }
    if (c < a.C) {
        float v = 0.f;
        for (int j = 0; j < k; ++j) {
            const int idx = oi[j];
            if (idx < 0 || idx >= a.Nb) continue;                  // a filler (fewer than k comparable similarities)
            if (a.labels[idx] == c) v += expf(os[j] * a.inv_temp); // a label outside [0, C) matches no thread: it votes for nobody
        }
        a.votes[(long)q * a.C + c] = v;
    }
}

int knn_check_shape(const char* who, int Q, int Nb, int k, int n_split) {
    GV_REQUIRE(Q >= 1, GV_E_SHAPE, "%s: need Q >= 1 (got %d)", who, Q);
    GV_REQUIRE(k >= 1 && k <= KMAXK, GV_E_SHAPE, "%s: need 1 <= k <= %d (got %d)", who, KMAXK, k);
    GV_REQUIRE(k <= Nb, GV_E_SHAPE, "%s: need k <= Nb (got k = %d, Nb = %d)", who, k, Nb);
    GV_REQUIRE(n_split >= 0 && n_split <= KMAXSPLIT && n_split <= Nb, GV_E_SHAPE,
               "%s: need 0 <= n_split <= min(%d, Nb) (got n_split = %d, Nb = %d)", who, KMAXSPLIT, n_split, Nb);
    return GV_OK;
}

// n_split = 0: enough splits to put a workgroup on every CU, each at least 1024 bank rows long
int knn_choose_split(int Q, int Nb, int n_split) {
    if (n_split > 0) return n_split;
    const int qt = (Q + KQT - 1) / KQT;
    int s = (gv_cu_budget() + qt - 1) / qt;
    s = min(s, max(1, Nb / 1024));
    return max(1, min(s, KMAXSPLIT));
}

GvLdsOptIn g_knn_lds;

}  // namespace

extern "C" int64_t gv_knn_workspace_bytes(int32_t Q, int32_t Nb, int32_t k, int32_t n_split) {
    if (knn_check_shape("gv_knn_workspace_bytes", Q, Nb, k, n_split) != GV_OK) return -1;
    return (int64_t)knn_choose_split(Q, Nb, n_split) * Q * k * 8;
}

extern "C" int gv_knn_vote(const gv_knn_vote_args* a, void* stream) {
    GV_REQUIRE(a && a->q && a->bank && a->labels && a->votes, GV_E_NULL, "gv_knn_vote: null pointer (q, bank, labels and votes are required)");
    int rc = knn_check_shape("gv_knn_vote", a->Q, a->Nb, a->k, a->n_split);
    if (rc != GV_OK) return rc;
    GV_REQUIRE(a->D >= 4 && a->D % 4 == 0 && a->D <= KMAXD, GV_E_SHAPE, "gv_knn_vote: need D a multiple of 4, 4 <= D <= %d (got %d)", KMAXD, a->D);
    GV_REQUIRE(a->C >= 1 && a->C <= KMAXC, GV_E_SHAPE, "gv_knn_vote: need 1 <= C <= %d (got %d)", KMAXC, a->C);
    GV_REQUIRE(a->ldq >= a->D && a->ldb >= a->D, GV_E_SHAPE, "gv_knn_vote: need ldq >= D and ldb >= D (got ldq = %lld, ldb = %lld, D = %d)",
               (long long)a->ldq, (long long)a->ldb, a->D);
    GV_REQUIRE(a->ldq % 4 == 0 && a->ldb % 4 == 0, GV_E_ALIGN, "gv_knn_vote: ldq and ldb must be multiples of 4 (got %lld, %lld)",
               (long long)a->ldq, (long long)a->ldb);
    GV_REQUIRE(gv_aligned(a->q, 16) && gv_aligned(a->bank, 16), GV_E_ALIGN, "gv_knn_vote: q and bank must be 16-byte aligned");
    KnnP p;
    p.a = *a;
    p.n_split = knn_choose_split(a->Q, a->Nb, a->n_split);
    p.per = (a->Nb + p.n_split - 1) / p.n_split;
    const int64_t need = (int64_t)p.n_split * a->Q * a->k * 8;
    GV_REQUIRE(a->workspace, GV_E_NULL, "gv_knn_vote: null workspace (%lld bytes needed, gv_knn_workspace_bytes)", (long long)need);
    GV_REQUIRE(a->workspace_bytes >= need, GV_E_SHAPE, "gv_knn_vote: workspace of %lld bytes, %lld needed (gv_knn_workspace_bytes)",
               (long long)a->workspace_bytes, (long long)need);
    GV_REQUIRE(gv_aligned(a->workspace, 4), GV_E_ALIGN, "gv_knn_vote: workspace must be 4-byte aligned");
    p.ws_sim = (float*)a->workspace;
    p.ws_idx = (int*)(p.ws_sim + (int64_t)p.n_split * a->Q * a->k);
    rc = gv_lds_opt_in(g_knn_lds, (const void*)knn_scan_kernel, knn_lds_bytes(KMAXK), "gv_knn_vote");
    if (rc != GV_OK) return rc;
    const unsigned qt = (unsigned)((a->Q + KQT - 1) / KQT);
    hipLaunchKernelGGL(knn_scan_kernel, dim3(qt, (unsigned)p.n_split), dim3(256), knn_lds_bytes(a->k), (hipStream_t)stream, p);
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)a->Q), dim3(256), 0, (hipStream_t)stream, p);
    GV_LAUNCH_CHECK("gv_knn_vote");
    return GV_OK;
}
