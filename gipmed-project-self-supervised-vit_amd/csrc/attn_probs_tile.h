// The arithmetic of the attention-probability kernels (gv_attention_probs in attention.hip, gv_attention_probs_stream in
// attention_probs_stream.hip): P = exp(scale q.k - lse[q]) with the forward's lse, one pass, no row reduction.
// S = Q K^T with queries on MFMA rows and keys on lanes: for a fixed (g, r) the 16 lanes li hold 16 consecutive keys of one
// query row, so each store instruction writes 4 rows x 64 contiguous bytes with 4-byte stores -- P rows start anywhere
// (N = 257: 1 028-byte rows), nothing is assumed about their alignment.  Each element is computed and stored as soon as its
// MFMA tile is done: no score registers are held across key tiles.
//
// Both files go through probs_rows / probs_keys, so a row of P has ONE expression in the tree: the two 16x16x32 MFMAs over
// d = 0..31 and 32..63, then exp2(fma(s, scale log2e, -lse log2e)).  Included inside each file's anonymous namespace, after
// attn_tiles.h.
#pragma once

constexpr float LOG2E = 1.4426950408889634f;

// what a lane keeps of one 16-query tile (rows q0 .. q0 + 15 of one (image, head) pair) across its key tiles
struct ProbsRows {
    bf16x8 qf[2];       // Q fragments of row q0 + li, d = 32 ks + 8 g ..
    float nl[4];        // -lse log2e of this lane's accumulator rows q0 + 4g + r
    bool qok[4];        // ... and whether they are < q_rows
    float c;            // scale log2e
    float* prow;        // p of row q0 + 4g (never dereferenced where qok is false)
};

__device__ __forceinline__ ProbsRows probs_rows(const gv_attention_probs_args& a, const bf16* qbase, long ld, long pair, int q0, int li, int g) {
    const int N = a.N, QR = a.q_rows;
    ProbsRows t;
    int qrow = q0 + li;
    qrow = qrow < QR ? qrow : QR - 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) t.qf[ks] = *(const bf16x8*)(qbase + (long)qrow * ld + ks * 32 + g * 8);
    // rows of this lane's accumulator: q0 + 4g + r; lse rows >= q_rows are never read
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + 4 * g + r;
        t.qok[r] = q < QR;
        t.nl[r] = -a.lse[pair * N + (t.qok[r] ? q : QR - 1)] * LOG2E;
    }
    t.c = a.scale * LOG2E;
    t.prow = a.p + (pair * QR + q0 + 4 * g) * (long)N;
    return t;
}

// the tile's 16 rows against the 16 keys key0 .. key0 + 15; k0 / k1: the K fragments (d = 8g .. / 32 + 8g ..) of key row key0 + li
__device__ __forceinline__ void probs_keys(const ProbsRows& t, int N, int key0, int li, bf16x8 k0, bf16x8 k1) {
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
    s = MFMA16(t.qf[0], k0, s);
    s = MFMA16(t.qf[1], k1, s);
    const int key = key0 + li;
    if (key < N) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (t.qok[r]) t.prow[(long)r * N + key] = __builtin_amdgcn_exp2f(fmaf(s[r], t.c, t.nl[r]));
    }
}

// one 16-query tile of one (image, head) pair against every key tile; kf(kt, ks) returns the K fragment of key row kt*16 + li.
// UNR: key tiles unrolled (NKT where the fragments sit in registers; 2 where they come from LDS: fully unrolled, the LDS reads
// of every tile are hoisted and 172 registers leave 2 waves per SIMD)
template <int NKT, int UNR, class KF>
__device__ __forceinline__ void probs_tile(const gv_attention_probs_args& a, const bf16* qbase, long ld, long pair, int q0, int li, int g, KF&& kf) {
    const ProbsRows t = probs_rows(a, qbase, ld, pair, q0, li, g);
#pragma unroll UNR
    for (int kt = 0; kt < NKT; ++kt) probs_keys(t, a.N, kt * 16, li, kf(kt, 0), kf(kt, 1));
}
