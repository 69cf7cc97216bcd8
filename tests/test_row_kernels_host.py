"""CPU: keeps the shape tables of tests/test_row_kernels_gpu.py honest.  That file restates the launch geometry of the row,
reduction and optimizer kernels in pure Python, with the caps read out of csrc/*.hip and include/gipvit.h as text; here every
parametrised shape is held to the property it was chosen for (a second trip with a ragged end, an odd slice count, a batch slice
of two rows with a short last one ...).  Retuning a launch either moves a number (a property below fails and names the table) or
rewrites the rule (the literal is no longer found and cap() names the tables to revisit)."""
import re

import pytest

import test_row_kernels_gpu as T


def test_every_launch_rule_is_still_in_the_source():
    for name, (_, _, today) in T._CAPS.items():
        assert T.cap(name) == today, f"{name}: the source now says {T.cap(name)}, the shape tables were chosen for {today}"


def test_a_missing_literal_names_the_shape_tables(monkeypatch):
    monkeypatch.setitem(T._CAPS, "no_such_rule", ("csrc/rowops.hip", r"blocks > (\d+) and a rule nobody wrote", (1,)))
    with pytest.raises(AssertionError, match=re.escape("revisit the shape tables of tests/test_row_kernels_gpu.py")):
        T.cap("no_such_rule")


def test_grid_stride_restatement():
    assert T.grid_stride(10, 4, 2048) == (1, 10)
    assert T.grid_stride(8192, 4, 2048) == (1, 8192)
    assert T.grid_stride(8193, 4, 2048) == (2, 1)
    assert T.grid_stride(3 * 8192, 4, 2048) == (3, 8192)


def test_layernorm_rows():
    per = 4 * T.cap("ln_fwd_grid")[0]
    assert [T.ln_fwd_trips(r)[0] for r in T.LN_FWD_ROWS] == [1, 2, 3], "LN_FWD_ROWS: no trip / second trip / third trip"
    assert T.ln_fwd_trips(T.LN_FWD_ROWS[0]) == (1, per), "LN_FWD_ROWS[0]: the control fills one trip exactly"
    for r in T.LN_FWD_ROWS[1:] + (T.LN_FWD_STRIDED_ROWS,):
        trips, last = T.ln_fwd_trips(r)
        assert trips >= 2 and last % 4, f"LN_FWD_ROWS {r}: a further trip that ends inside a workgroup"
    assert max(T.ln_fwd_trips(r)[0] for r in (1003, 40)) == 1, "the shapes of tests/test_kernels_gpu.py never prefetch"
    assert [T.ln_bwd_trips(r)[0] for r in T.LN_BWD_ROWS] == [1, 2, 3], "LN_BWD_ROWS"
    assert T.ln_bwd_trips(T.LN_BWD_ROWS[0])[1] == 4 * T.cap("ln_partial_blocks")[0]
    for r in T.LN_BWD_ROWS[1:]:
        assert T.ln_bwd_trips(r)[1] % 4, f"LN_BWD_ROWS {r}: ragged last trip"
    assert all(T.ln_bwd_idle_blocks(r) == 0 for r in T.LN_BWD_ROWS) and T.ln_bwd_idle_blocks(T.LN_BWD_IDLE_ROWS) > 1000
    assert {v[0] for v in T.LN_BWD_VARIANTS} == set(T.LN_BWD_ROWS) | {T.LN_BWD_IDLE_ROWS}
    assert {v[1] for v in T.LN_BWD_VARIANTS} == {True, False} and {v[2] for v in T.LN_BWD_VARIANTS} == {True, False}
    assert any(v[3] for v in T.LN_BWD_VARIANTS) and any(v[4] for v in T.LN_BWD_VARIANTS)


def test_finalizer_blocks():
    nz = T.cap("ln_finalize_slices")[0]
    shapes = {n: T.ln_finalize_slices(n) for n in T.FINALIZE_BLOCKS}
    assert any(used < nz for _, used, _ in shapes.values()), "FINALIZE_BLOCKS: a count that leaves ln_finalize slices empty"
    assert any(per > 1 and last < per for per, _, last in shapes.values()), "FINALIZE_BLOCKS: a ragged last ln_finalize slice"
    assert shapes[T.cap("ln_partial_blocks")[0]] == (T.cap("ln_partial_blocks")[0] // nz, nz, T.cap("ln_partial_blocks")[0] // nz)
    # colsum_finalize: group grp takes blocks grp, grp + 4 as a pair, stepping by 8, then one odd block
    def tail(n, grp):
        b = grp
        while b + 4 < n:
            b += 8
        return b < n
    assert any(tail(n, 0) for n in T.FINALIZE_BLOCKS) and any(not tail(n, 0) for n in T.FINALIZE_BLOCKS if n > 4), "odd tail taken and not taken"
    assert any(n < 4 for n in T.FINALIZE_BLOCKS), "fewer blocks than row groups"
    assert 2 in T.FINALIZE_CS and any(c % 64 == 0 and c > 64 for c in T.FINALIZE_CS)


def test_colsum_rows():
    big, per16, n_big, _, _ = T.cap("colsum_slices")
    sl = {r: T.colsum_slices(r) for r in T.COLSUM_ROWS}
    assert sl[36][0] == 3 and sl[196][0] == 13, "the engine's 36- and 196-row calls: odd slice counts"
    assert any(n == 1 and r < per16 for r, (n, _, _) in sl.items()), "COLSUM_ROWS: fewer rows than one slice holds"
    assert big * per16 - 1 in T.COLSUM_ROWS and big * per16 in T.COLSUM_ROWS, "COLSUM_ROWS: both sides of the slice-rule threshold"
    assert any(n == n_big and last < per for n, per, last in sl.values()), "COLSUM_ROWS: 64 slices with a short last one"
    assert any(per % 4 for _, per, _ in sl.values()), "COLSUM_ROWS: a slice that is no multiple of the four waves"
    cols = T.cap("colsum_cols")[0]
    assert any(c < cols for c in T.COLSUM_CS) and any(c > cols and c % cols for c in T.COLSUM_CS) and any(c % cols == 0 for c in T.COLSUM_CS)


def test_sumsq_sizes():
    pieces = {n: T.sumsq_pieces(n) for n in T.SUMSQ_NS}
    assert pieces[T.SUMSQ_NS[0]][:3] == (0, 0, 0) and pieces[T.SUMSQ_NS[0]][3] == 3, "SUMSQ_NS[0]: the scalar tail alone"
    assert T.sumsq_pieces(1_000_003)[0] == 0, "the shape of tests/test_kernels_gpu.py never enters the two-piece loop"
    assert pieces[1 << 20][0] == 0 and pieces[(1 << 20) + 4][0] == 1, "SUMSQ_NS: both sides of the two-piece loop's threshold"
    two, trips, rem, tail = pieces[T.SUMSQ_NS[-1]]
    stride = 256 * T.cap("sumsq_grid")[0]
    assert two == stride and trips == 1 and 0 < rem < stride and tail == 3, "SUMSQ_NS[-1]: every thread loops, some take the remainder, a tail"


def test_elementwise_sizes():
    trips, last, tail = T.cast_trips(T.CAST_N)
    assert trips == 2 and 0 < last < 256 * T.cap("cast_grid")[0] and last % 256 and tail, "CAST_N"
    assert T.cast_trips(1_000_003)[0] == 1
    trips, last = T.dropout_trips(T.DROPOUT_N)
    assert trips == 2 and last % 256, "DROPOUT_N"
    rows, cols = T.DROPOUT_ADD_SHAPE
    trips, last = T.dropout_trips(rows * cols, add=True)
    assert trips == 2 and 0 < last < cols, "DROPOUT_ADD_SHAPE: the second trip lies inside the last row"
    assert T.adam_trips(T.ADAM_TRIP_N) == (2, 777) and T.ADAM_TRIP_N % 4 == 0, "ADAM_TRIP_N"
    assert T.adam_trips(T.ADAM_N)[0] == 1 and T.adam_trips(135168)[0] == 1
    assert any(k < 256 for k in T.CENTER_KS) and any(k > 256 and k % 256 for k in T.CENTER_KS)


def test_token_shapes():
    per = T.cap("tok_img_per_chunk")[0]
    ch = [T.tok_chunks(i) for i in T.TOK_IMGS]
    assert ch[0] == (1, per), "TOK_IMGS[0]: one full chunk"
    assert any(c == 2 and last == 1 for c, last in ch) and any(c >= 3 and 1 < last < per for c, last in ch), "TOK_IMGS: ragged last chunks"
    assert T.tok_chunks(6)[0] == 1, "the shape of tests/test_kernels_gpu.py is one chunk"
    assert any(d < 256 for d in T.TOK_DS) and any(d > 512 for d in T.TOK_DS) and 2 in T.TOK_NS


def test_small_matmul_shapes():
    u = T.cap("small_matmul_unroll")[0]
    cols = T.cap("small_matmul_cols")[0]
    assert {1, u - 1, u, u + 1} <= set(T.SMM_KS) and any(k > 2 * u and k % u for k in T.SMM_KS)
    assert any(n < cols for n in T.SMM_NS) and cols in T.SMM_NS and any(cols < n < 2 * cols for n in T.SMM_NS)
    assert 1 in T.SMM_MS and any(m > 1 for m in T.SMM_MS)


def test_norm_shapes():
    per = T.cap("row_loop_cols")[0]
    trips = {c: T.row_loop_trips(c) for c in T.NORM_CS}
    assert trips[per] == (1, per) and any(t == 2 and last == 4 for t, last in trips.values()), "NORM_CS: one lane alone in a second trip"
    assert any(t == 3 and last == per for t, last in trips.values()) and any(t == 2 and 4 < last < per for t, last in trips.values())
    assert any(t == 1 and last == 4 for t, last in trips.values())
    assert any(r % 4 for r in T.NORM_ROWS) and 1 in T.NORM_ROWS
    # the C = 256 kernels: wave w of workgroup g takes rows 8 g + w and 8 g + w + 4
    second = {r: [(r0 + 4) < r for r0 in range(0, r) if r0 % 8 < 4] for r in T.WN256_ROWS}
    assert any(all(v) for v in second.values()) and any(not any(v) for v in second.values()) and any(any(v) and not all(v) for v in second.values())


def test_dino_cases():
    sp = {c: T.dino_split(c[0], c[3]) for c in T.DINO_CASES}
    assert any(b_per >= 2 and last < b_per for _, _, b_per, last in sp.values()), "DINO_CASES: a batch loop with a short last slice"
    for B, V, G, K in ((4, 10, 2, 4096), (3, 4, 2, 256), (2, 2, 2, 65536), (5, 6, 1, 1024)):
        assert T.dino_split(B, K)[2] == 1, "the shapes of tests/test_kernels_gpu.py never loop over the batch"
    assert {g for _, _, g, _ in T.DINO_CASES} >= {1, 2, 3, 4} and any(v == 16 for _, v, _, _ in T.DINO_CASES)
    assert any(v == g for _, v, g, _ in T.DINO_CASES) and any(k == 4 for *_, k in T.DINO_CASES)
    assert all(k % 4 == 0 and 2 <= v <= 16 and 1 <= g <= min(4, v) for _, v, g, k in T.DINO_CASES), "every case passes gv_dino_loss's checks"
    rs = {k: T.row_stats_trips(k) for *_, k in T.DINO_CASES}
    assert any(t == 1 and inside > 0 and outside > 0 for t, inside, outside in rs.values()), "a second piece partly outside the row"
    assert any(t == 2 and inside == 0 and outside == 1 for t, inside, outside in rs.values()), "a second trip of one thread"
    assert any(k % T.cap("dino_kblock")[0] for *_, k in T.DINO_CASES)
    assert T.DINO_OPTIONS_CASE in T.DINO_CASES and T.DINO_INT_TEACHER_CASE in T.DINO_CASES


def test_lsce_shapes():
    assert 64 in T.LSCE_CS and 1 in T.LSCE_CS and {1, 256, 257} <= set(T.LSCE_BS)
