"""The rANS / tANS launch-path cases (tests/rans_cases.py, tests/tans_cases.py) on the CPU: every case is sound in the oracle,
sits on the kernel it names by the thresholds of the library restated, and together they name every kernel of both enums of
include/basic_hip.h -- which is what keeps tests/test_gpu_rans_paths.py from skipping a path quietly.  Also the power of the
precision sweep: an exact-integer encoder with the fast kernel's 24-bit multiply differs from the oracle exactly below p = 7."""
import numpy as np
import pytest

import rans_cases as rc
import tans_cases

ALL = rc.names()


@pytest.mark.parametrize("name", ALL)
def test_case_round_trips_in_the_oracle(oracle, name):
    """Bytes within the oracle's 2n + 8 words (it raises past them); decoding them gives the symbols back and ends at state
    2^31 with every word read -- the GPU decode tests assert the same of d_state / d_pos."""
    c = rc.case(name)
    streams = rc.oracle_streams(name)
    assert len(streams) == len(c.streams) and len(c.streams) in (rc.BATCH, rc.RESUME_IMAGES * rc.RESUME_LANES)
    _, dec = rc.oracle_coders(c)
    for i, ((sym, idx), words) in enumerate(zip(c.streams, streams)):
        assert 2 <= words.size <= 2 * idx.size + 8, (i, words.size)
        if c.ar is not None:
            back = dec.decode_with_indexes(words.tobytes(), idx, ar_indexes=np.zeros_like(idx), ar_offsets=c.ar_offsets(idx.size))
            assert np.array_equal(back, sym), i
            continue
        (back, state, pos), = rc.oracle_decode_pieces(c, words, idx, [idx.size])
        assert np.array_equal(back, sym), i
        assert state == 1 << 31 and pos == words.size, (i, state, pos, words.size)


def test_stream_shapes():
    for c in rc.all_cases():
        lens = [idx.size for _, idx in c.streams]
        if c.name.startswith("resume_"):
            assert lens == [rc.RESUME_LEN] * 15 and c.bypass
            continue
        want = list(rc.BATCH_LENGTHS)
        if c.name == "extreme16":
            want[10] = want[rc.FREQ1_STREAM] = 5000
        assert lens == want and set(rc.LENGTHS) <= set(lens) and len(lens) == 19, c.name
    for w in rc.WAVES[1:]:
        assert rc.BATCH % w      # a part-filled last workgroup at every W above 1


def test_extreme_tables_hold_the_edges(oracle):
    c = rc.case("extreme16")
    freq = np.concatenate([np.diff(c.cdfs[r, : c.sizes[r]]) for r in range(len(c.sizes))])
    assert {1, 65535, 32768} <= set(freq.tolist()) and 65535 in c.cdfs[0].tolist()     # a start of 2^p - 1
    sym, idx = c.streams[rc.FREQ1_STREAM]
    f = np.array([c.cdfs[r, s - c.offsets[r] + 1] - c.cdfs[r, s - c.offsets[r]] for s, r in zip(sym.tolist(), idx.tolist())])
    assert (f == 1).all() and set(idx.tolist()) == {0, 1, 3}
    assert rc.oracle_streams("extreme16")[rc.FREQ1_STREAM].size == 2502     # 16 bits a symbol: a word every second symbol
    # every row and every symbol of the table is coded somewhere
    used = {(int(r), int(v - c.offsets[r])) for sy, ix in c.streams for v, r in zip(sy.tolist(), ix.tolist())}
    assert used == {(r, v) for r in range(len(c.sizes)) for v in range(c.sizes[r] - 1)}
    b = rc.case("extreme16_bypass")
    sent = sorted({int(b.cdfs[r, b.sizes[r] - 1] - b.cdfs[r, b.sizes[r] - 2]) for r in range(len(b.sizes))})
    assert sent[0] == 1 and (1 << 16) - 39 in sent
    raw = []
    for sy, ix in b.streams:
        v = sy.astype(np.int64) - b.offsets[ix]
        mx = b.sizes[ix] - 2
        raw += np.where(v < 0, -2 * v - 1, np.where(v >= mx, 2 * (v - mx), -1)).tolist()
    raw = np.array(raw)
    assert (raw >= 1 << 30).any() and (raw < 1 << 31).all() and ((raw >= 0) & (raw < 8)).any() and (raw == -1).any()


def test_lowp_and_width_tables():
    for p in rc.LOWP:
        c = rc.case(f"lowp{p}")
        assert c.precision == p and c.sizes.tolist() == [min(1 << p, 5) + 1] * 3 + [2] and c.cdfs[3, :2].tolist() == [0, 1 << p]
        assert all(3 in idx.tolist() for _, idx in c.streams if idx.size > 60)      # the zero-bit row is coded
    assert rc.case("row_widths").sizes.tolist() == [2, 3, 63, 64, 65, 66, 128, 129, 4096]
    assert rc.case("row_widths_4097").sizes.tolist() == [2, 3, 63, 64, 65, 66, 128, 129, 4096, 4097]
    assert rc.case("image_too_big").sizes.tolist() == [4096] * 10 and rc.image_bytes(rc.case("image_too_big")) == 166560 + 1024
    assert rc.packed_bytes(rc.case("image_too_big")) == 80 * 1024
    assert rc.case("global_tables").sizes.tolist() == [4098] * 18 and rc.packed_bytes(rc.case("global_tables")) > 144 * 1024
    z = rc.case("zero_width")
    assert z.cdfs.tolist() == [[0, 100, 100, 65536]]
    assert all(1 not in (sym - z.offsets[0]).tolist() for sym, _ in z.streams)       # the zero-width symbol is never coded
    for name in ("row_widths", "row_widths_4097"):      # nor is the 2-entry row, whose frequency is 0 after the uint16 cast
        assert all(0 not in idx.tolist() for _, idx in rc.case(name).streams)
    for name in ("row_widths_4097", "global_tables", "image_too_big"):                 # the widest rows are coded to their last symbol
        c = rc.case(name)
        r = int(np.argmax(c.sizes))
        vals = np.concatenate([(sym - c.offsets[idx])[idx == r] for sym, idx in c.streams])
        assert vals.max() > c.sizes[r] - 2 - 64 and vals.min() < 64


@pytest.mark.parametrize("name", ALL)
def test_case_sits_on_the_kernel_it_names(name):
    c = rc.case(name)
    assert rc.predict(c) == (c.enc, c.dec)


def test_thresholds_from_both_sides():
    assert (rc.case("rows2049").enc, rc.case("rows2048").enc) == ("ENC_GENERAL", "ENC_FAST")
    assert len(rc.case("rows2049").sizes) == 2049 and len(rc.case("rows2048").sizes) == 2048
    assert (rc.case("row_widths").dec, rc.case("row_widths_4097").dec) == ("DEC_FAST", "DEC_GENERAL_LDS")
    assert rc.image_bytes(rc.case("row_widths")) <= rc.FAST_IMAGE_BUDGET < rc.image_bytes(rc.case("image_too_big"))
    assert rc.packed_bytes(rc.case("row_widths_4097")) <= rc.LDS_TABLE_BUDGET < rc.packed_bytes(rc.case("global_tables"))
    assert [rc.case(f"lowp{p}").enc for p in rc.LOWP] == ["ENC_GENERAL"] * 4 + ["ENC_FAST"] * 4
    assert [rc.case(f"lowp{p}").dec for p in rc.LOWP] == ["DEC_GENERAL_LDS"] * 4 + ["DEC_FAST"] * 4
    assert [tans_cases.path_kernels(L, nd) for L, nd in tans_cases.PATH_CONFIGS] == [
        ("ENC_LDS", "DEC_LDS"), ("ENC_LDS", "DEC_GLOBAL"), ("ENC_LDS", "DEC_GLOBAL"), ("ENC_GLOBAL", "DEC_GLOBAL"), ("ENC_LDS", "DEC_LDS")]


def test_every_kernel_of_both_enums_is_named():
    rans = rc.header_enum("BASIC_RANS_KERNEL_")
    assert sorted(rans.values()) == list(range(8))
    named = set().union(*(c.kernels for c in rc.all_cases()))
    assert named == set(rans)
    tans = rc.header_enum("BASIC_TANS_KERNEL_")
    assert sorted(tans.values()) == list(range(4))
    assert set().union(*(tans_cases.path_kernels(L, nd) for L, nd in tans_cases.PATH_CONFIGS)) == set(tans)
    from cbench_basic_amd import ans
    from cbench_basic_amd.nn import kernels
    assert {n: getattr(kernels, "RANS_KERNEL_" + n) for n in rans} == rans and kernels.RANS_KERNEL_NONE == -1
    assert {n: getattr(ans, "TANS_KERNEL_" + n) for n in tans} == tans and ans.TANS_KERNEL_NONE == -1


@pytest.mark.parametrize("p", rc.LOWP)
def test_python_encoder_and_the_24_bit_cut(oracle, p):
    """The exact-integer encoder equals the oracle at every precision.  With the quotient's high word cut to 24 bits, as in the
    fast kernel's v_mad_u32_u24, it differs below p = 7 and not from there on (q < 2^(63-p), high word < 2^(31-p)): the lowp
    cases can tell such a kernel from a correct one."""
    c = rc.case(f"lowp{p}")
    streams = rc.oracle_streams(c.name)
    differs = []
    for (sym, idx), words in zip(c.streams, streams):
        assert np.array_equal(rc.python_encode(c, sym, idx), words)
        differs.append(not np.array_equal(rc.python_encode(c, sym, idx, cut24=True), words))
    if p < rc.FAST_MIN_PRECISION:
        assert differs[rc.LENGTHS.index(4097)] and sum(differs) >= 4, differs
    else:
        assert not any(differs), differs


@pytest.mark.parametrize("p", rc.LOWP)
def test_python_decoder_and_the_24_bit_cut(oracle, p):
    """The same for the decoder: the wave decoder's generic path multiplies the high word of x >> p (below 2^(31-p)) as a 24-bit
    operand.  Exact integers decode every stream and end at state 2^31 with every word read; with the cut, wrong symbols below
    p = 7 and none from there on."""
    c = rc.case(f"lowp{p}")
    wrong = []
    for (sym, idx), words in zip(c.streams, rc.oracle_streams(c.name)):
        back, state, pos = rc.python_decode(c, words, idx)
        assert np.array_equal(back, sym) and state == 1 << 31 and pos == words.size
        wrong.append(not np.array_equal(rc.python_decode(c, words, idx, cut24=True)[0], sym))
    if p < rc.FAST_MIN_PRECISION:
        assert wrong[rc.LENGTHS.index(4097)] and sum(wrong) >= 4, wrong
    else:
        assert not any(wrong), wrong


@pytest.mark.parametrize("L,nd", tans_cases.PATH_CONFIGS)
def test_tans_path_cases_in_the_oracle(L, nd):
    from oracle import tans_oracle
    cases = tans_cases.path_case(L, nd)
    assert len(cases) == tans_cases.PATH_STREAMS and sorted(c[6].size for c in cases)[:2] == [0, 1]
    kept = 0
    for c in cases:
        data, coded, back = tans_cases.run_raw(tans_oracle, c)
        assert len(data) >= 1 and data[-1] != 0 and coded >= c[6].size and np.array_equal(back, c[5])
        err, budgeted, _ = tans_cases.run(tans_oracle, c)      # the reference's budget rule: the same bytes, none, or its error
        assert (err is not None and c[6].size * L // 8 <= 8) or budgeted in (data, b"")
        kept += budgeted == data
    assert kept >= 20
