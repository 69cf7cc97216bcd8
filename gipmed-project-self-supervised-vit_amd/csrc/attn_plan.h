// Which kernel an attention call gets and with what launch geometry -- gv_attention_fwd / _bwd / _probs, the varlen calls and
// gv_attention_fwd_stream / gv_attention_bwd_stream / gv_attention_probs_stream (include/gipvit.h).  This is the ONE place where the
// length classes, the per-class workgroup shapes, the dynamic LDS sizes and the occupancy promises are stated: the kernels of
// attention.hip / attention_stream.hip / attention_stream_bwd.hip / attention_probs_stream.hip take their
// constants from the Cfg structs below, the launchers launch the Launch the same structs give.  Pure host C++17, no HIP: the
// header compiles with a plain g++ (tests/attn_plan_main.cc replays tests/traces/attention_plans.json through it).
#pragma once
#include "../../include/gipvit.h"
#include <utility>

namespace gvattn {

constexpr int ROW = 128;                                    // bytes of one token row of the LDS image: 64 d, 16 bit (attn_tiles.h)
constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }
struct Launch { long grid; int block, lds_bytes; };         // workgroups, threads per workgroup, dynamic LDS

// what every entry point asks of its shape (max_n: GV_ATTN_MAX_N, or GV_ATTN_STREAM_MAX_N for the streaming calls)
constexpr bool shape_ok(int n_img, int H, int N, int max_n) { return n_img > 0 && H > 0 && N > 0 && N <= max_n; }

// ---------------------------------------------------------------------------------
// length classes: a sequence of N tokens runs in the smallest class NKT (16-key tiles, the kernels' template argument) that holds it
// ---------------------------------------------------------------------------------
using Classes = std::integer_sequence<int, 2, 4, 8, 14, 18>;
static_assert(16 * 18 == GV_ATTN_MAX_N, "the largest class is the entry points' limit");

template <class F, int C0, int... C>
auto with_class_of(int N, F&& f, std::integer_sequence<int, C0, C...>) {
    if constexpr (sizeof...(C) == 0) return f(std::integral_constant<int, C0>{});
    else return N <= 16 * C0 ? f(std::integral_constant<int, C0>{}) : with_class_of(N, f, std::integer_sequence<int, C...>{});
}
// f(std::integral_constant<int, NKT>{}) for the class of N (0 < N <= GV_ATTN_MAX_N: the entry points have checked it)
template <class F> auto with_class(int N, F&& f) { return with_class_of(N, f, Classes{}); }
inline int class_of(int N) { return with_class(N, [](auto c) { return (int)decltype(c)::value; }); }

// ---------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------
template <int NKT>
struct FwdCfg {
    // long sequences: 16 queries per wave and round (the score registers halve, two 8-wave workgroups
    // fit a CU and cover each other's load phases); short ones: 32 queries per wave
    static constexpr int QT = NKT >= 14 ? 1 : 2;                  // 16-query tiles per wave and round
    static constexpr int NQB = (NKT + QT - 1) / QT;               // query blocks of 16 QT rows
    static constexpr int NW = NQB >= 5 ? 8 : 4;                   // waves per workgroup
    static constexpr int PAIRS = NQB >= NW ? 1 : (NW / NQB >= 1 ? NW / NQB : 1);
    static constexpr int WPP = NW / PAIRS;                        // waves per (image, head) pair
    static constexpr int ROUNDS = (NQB + WPP - 1) / WPP;          // query blocks per wave
    static constexpr int NP = NKT * 16;                           // token rows of an image
    static constexpr int IMG = NP * ROW;                          // one K or V image
    static constexpr int LDS = PAIRS * 2 * IMG;
    static constexpr int THREADS = NW * 64;
    // waves per SIMD the register allocation must leave room for: two 8-wave workgroups per CU = 4
    static constexpr int OCC = QT == 1 && NKT <= 14 ? 4 : (QT == 1 ? 2 : 1);
};
template <int NKT> Launch fwd_launch(int n_pairs) { return {ceil_div(n_pairs, FwdCfg<NKT>::PAIRS), FwdCfg<NKT>::THREADS, FwdCfg<NKT>::LDS}; }

// Varlen forward: a two-segment table of a long (class 14) and a short (class 4) segment, either order, runs as ONE launch of
// 8-wave workgroups -- the first long_blocks() run the long class, each of the rest runs SHORT_PER_WG 4-wave instances of the short
// class side by side in their own LDS parts (attn_fwd_varlen_kernel)
struct VarlenCfg {
    static constexpr int LONG = 14, SHORT = 4;
    static constexpr bool fuses(int class_a, int class_b) { return class_a == LONG && class_b == SHORT; }
    static constexpr int SHORT_PER_WG = FwdCfg<LONG>::NW / FwdCfg<SHORT>::NW;
    static_assert(FwdCfg<LONG>::NW == 8 && FwdCfg<SHORT>::NW == 4, "varlen launch: 8-wave long class, two 4-wave short instances");
    static constexpr int LDS_SHORT = FwdCfg<SHORT>::LDS;
    static constexpr int LDS = FwdCfg<LONG>::LDS > SHORT_PER_WG * LDS_SHORT ? FwdCfg<LONG>::LDS : SHORT_PER_WG * LDS_SHORT;
    static constexpr int THREADS = FwdCfg<LONG>::THREADS, OCC = FwdCfg<LONG>::OCC;
    static constexpr int long_blocks(int np_long) { return ceil_div(np_long, FwdCfg<LONG>::PAIRS); }
    static Launch launch(int np_long, int np_short) {
        return {long_blocks(np_long) + ceil_div(np_short, SHORT_PER_WG * FwdCfg<SHORT>::PAIRS), THREADS, LDS};
    }
};
// the long segment (0 / 1) of a two-segment table that fuses, -1 for one that does not
inline int varlen_long_segment(int N0, int N1) {
    const int c0 = class_of(N0), c1 = class_of(N1);
    return VarlenCfg::fuses(c0, c1) ? 0 : (VarlenCfg::fuses(c1, c0) ? 1 : -1);
}

// ---------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------
// KT = 16-key tiles per wave.  KT = 2: 32 keys per wave, ~190 registers, 2 waves per SIMD.  KT = 1: 16 keys per wave, the same
// chain on half the keys in < 128 registers, 4 waves per SIMD -- but every wave still reads all of Q and dO from LDS, so the
// workgroup's LDS read traffic of phase A doubles (measured: the short crops gain 20 %, N = 197 gains nothing; see bwd_kt).
template <int NKT, int KT>
struct BwdCfg {
    static constexpr int NKB = NKT / KT;               // key blocks of 16 KT keys = waves per pair
    static constexpr int PAIRS = NKB >= 4 ? 1 : 4 / NKB;
    static constexpr int NW = NKB * PAIRS;             // waves per workgroup
    // dS^T images.  2 where a (image, head) pair holds its CU alone anyway (N = 197: 142 KB instead of 114): the image alternates per
    // 64-query step and the step's second barrier goes (72.9 -> 70.4 us per launch; the short classes, several workgroups per CU, keep 1)
    static constexpr int NDS = NKT == 14 ? 2 : 1;
    static constexpr int NP = NKT * 16;
    static constexpr int IMG = NP * ROW;               // one Q, K or dO image
    static constexpr int QH = NKT >= 8 ? 2 : 1;        // 32-query halves per barrier pair (short sequences keep 1)
    static constexpr int DROW = 64 * QH;               // dS^T image: [key][32 QH q] bf16
    static constexpr int DST = NP * DROW;
    static constexpr int PER_PAIR = 3 * IMG + NDS * DST + 2 * NP * 4;      // Q, K, dO; dS^T; delta and lse
    static constexpr int LDS = PAIRS * PER_PAIR;
    static constexpr int THREADS = NW * 64;
    // short sequences run two 4-wave workgroups per CU: the second launch-bounds argument keeps them within 256 registers
    static constexpr int OCC = (NKT >= 14 || NW > 8) ? 1 : 2;
    static_assert(THREADS <= 1024 && LDS <= 160 * 1024, "workgroup size / LDS");
};
// keys per wave: 16 for the short crops (N = 37: 39.2 -> 31.4 us per launch of 512 images x 6 heads), 32 from N = 65 on (N = 197:
// 72.6 us against 73.8 with 16 -- twice the waves buy nothing there: per (image, head) pair the kernel is the SUM of ~8 us of
// exp / dS arithmetic, ~4 us of MFMA and ~8 us (32 keys) or ~12 us (16 keys) of LDS reads, phase-aligned by its barriers)
constexpr int bwd_kt(int NKT) { return NKT == 4 ? 1 : 2; }
template <int NKT> using BwdOf = BwdCfg<NKT, bwd_kt(NKT)>;
template <int NKT> Launch bwd_launch(int n_pairs) { return {ceil_div(n_pairs, BwdOf<NKT>::PAIRS), BwdOf<NKT>::THREADS, BwdOf<NKT>::LDS}; }

// ---------------------------------------------------------------------------------
// attention probabilities: q_rows <= PROBS_ROW_Q (the CLS row) runs the row kernel, one wave per pair and no LDS; more rows run
// one workgroup per pair with K staged once, the pair's 16-query tiles spread over up to PROBS_NW waves
// ---------------------------------------------------------------------------------
constexpr int PROBS_NW = 4, PROBS_ROW_Q = 16;
constexpr bool probs_by_row(int q_rows) { return q_rows <= PROBS_ROW_Q; }
template <int NKT> Launch probs_launch(int n_pairs, int q_rows) {
    if (probs_by_row(q_rows)) return {ceil_div(n_pairs, PROBS_NW), PROBS_NW * 64, 0};
    const int n_qt = ceil_div(q_rows, 16);
    return {n_pairs, (n_qt < PROBS_NW ? n_qt : PROBS_NW) * 64, FwdCfg<NKT>::IMG};
}

// ---------------------------------------------------------------------------------
// streaming forward: a workgroup = one pair x one block of QB query rows, K / V double buffered in blocks of KB keys
// ---------------------------------------------------------------------------------
struct StreamCfg {
    static constexpr int QB = GV_ATTN_STREAM_QBLOCK;    // query rows per workgroup
    static constexpr int NW = 4;                        // waves per workgroup
    static constexpr int KB = 64;                       // keys per block
    static constexpr int IMG = KB * ROW;                // one K or V block image
    static constexpr int LDS = 2 * 2 * IMG;             // two stages of (K, V)
    static constexpr int THREADS = NW * 64, OCC = 4;    // four workgroups per CU cover each other's barriers
    static_assert(GV_ATTN_STREAM_MAX_N % 16 == 0 && LDS <= 160 * 1024, "key tiles / LDS");
    // q_limit > 0: whole query blocks that hold a row < q_limit
    static constexpr int query_blocks(int N, int q_limit) { return ceil_div(q_limit > 0 && q_limit < N ? q_limit : N, QB); }
    static Launch launch(int n_img, int H, int N, int q_limit) { return {(long)n_img * H * query_blocks(N, q_limit), THREADS, LDS}; }
};

// ---------------------------------------------------------------------------------
// streaming backward (gv_attention_bwd_stream): two launches, the second behind the first on the stream
//   dQ:       a workgroup = one pair x one block of QB query rows (the forward's shape), K / V double buffered in blocks of KB keys;
//             it also writes delta.  Every query block of the sequence has a workgroup: those behind q_limit store zeros.
//   dK / dV:  a workgroup = one pair x one block of KEYS keys, Q / dO (+ lse / delta) double buffered in blocks of QS query rows
// ---------------------------------------------------------------------------------
struct StreamBwdCfg {
    static constexpr int QB = StreamCfg::QB, NW = StreamCfg::NW, KB = StreamCfg::KB;
    static constexpr int IMG = KB * ROW;                        // one K or V block image (dQ launch)
    static constexpr int LDS_DQ = 2 * 2 * IMG;                  // two stages of (K, V)
    static constexpr int KEYS = 32 * NW;                        // dK / dV launch: 32 keys per wave
    static constexpr int QS = 64;                               // query rows per stage
    static constexpr int QIMG = QS * ROW;                       // one Q or dO stage image
    static constexpr int ROWV = 2 * QS * 4;                     // lse and delta of a stage's rows, f32
    static constexpr int STAGE = 2 * QIMG + ROWV;
    static constexpr int LDS_DKV = 2 * STAGE;
    static constexpr int THREADS = NW * 64;
    static constexpr int OCC_DQ = 2, OCC_DKV = 2;               // waves per SIMD the register allocation leaves room for
    static_assert(QB == 32 * NW && KB % 32 == 0 && QS % 32 == 0 && QS == 64, "32 rows per wave; one wave stages a stage's lse or delta");
    static_assert(LDS_DQ * (OCC_DQ * 4 / NW) <= 160 * 1024 && LDS_DKV * (OCC_DKV * 4 / NW) <= 160 * 1024, "LDS of the promised workgroups per CU");
    // query rows the call reads: whole QB-row blocks that hold a row < q_limit (what gv_attention_fwd_stream computed)
    static constexpr int query_end(int N, int q_limit) {
        return q_limit > 0 && ceil_div(q_limit, QB) * QB < N ? ceil_div(q_limit, QB) * QB : N;
    }
    static Launch launch_dq(int n_img, int H, int N) { return {(long)n_img * H * ceil_div(N, QB), THREADS, LDS_DQ}; }
    static Launch launch_dkv(int n_img, int H, int N) { return {(long)n_img * H * ceil_div(N, KEYS), THREADS, LDS_DKV}; }
};

// ---------------------------------------------------------------------------------
// streaming attention probabilities (gv_attention_probs_stream): the sequence is never resident
//   row form   (q_rows <= PROBS_ROW_Q, the CLS row): a workgroup = one pair; its 16-key tiles are dealt to the ROW_NW waves in
//              chunks of ROW_CH tiles whose K fragments come straight from global, all issued before the chunk's first MFMA.  No LDS.
//   block form (more rows): a workgroup = one pair x one block of QB query rows (the streaming forward's shape, Q fragments in
//              registers), K double buffered in blocks of KB keys.  Only the blocks that hold a row < q_rows are launched.
// ---------------------------------------------------------------------------------
struct ProbsStreamCfg {
    static constexpr int ROW_NW = 4, ROW_CH = 8;                // row form: waves per workgroup, 16-key tiles per chunk (64 registers)
    static constexpr int ROW_THREADS = ROW_NW * 64, ROW_OCC = 2;
    static constexpr int QB = StreamCfg::QB, NW = StreamCfg::NW, KB = StreamCfg::KB;
    static constexpr int IMG = KB * ROW;                        // one K block image
    static constexpr int LDS = 2 * IMG;                         // two stages of K
    static constexpr int THREADS = NW * 64, OCC = 4;            // four workgroups per CU cover each other's barriers and stores
    static_assert(QB == 32 * NW && KB % 16 == 0 && LDS * OCC <= 160 * 1024, "32 rows per wave; key tiles; LDS of the promised workgroups per CU");
    static constexpr bool by_row(int q_rows) { return probs_by_row(q_rows); }
    static constexpr int query_blocks(int q_rows) { return ceil_div(q_rows, QB); }
    static Launch launch(int n_img, int H, int q_rows) {
        const long pairs = (long)n_img * H;
        return by_row(q_rows) ? Launch{pairs, ROW_THREADS, 0} : Launch{pairs * query_blocks(q_rows), THREADS, LDS};
    }
};

}  // namespace gvattn
