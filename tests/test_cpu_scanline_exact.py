"""The premises of the exact scan-line reference (scanline_exact.py), checked without a GPU: its arithmetic is exact in fp32 in any
order, its inputs sit on the ties continuous inputs never reach, and it has power -- a wrong causal window changes what it codes."""
import numpy as np
import pytest

from scanline_exact import TABLE, causal_taps, exact_case, exact_params, reference

SHAPE = (1, 5, 7)   # B, H, W: every tap of a 5 x 5 window lies inside the image somewhere, and outside it somewhere
SEED = 57


@pytest.mark.parametrize("ks", [5, 3])
def test_arithmetic_is_exact_in_fp32(ks):
    """Every intermediate (context sums, the merger's pre-activations, the coded latent) is non-negative -- LeakyReLU is the
    identity --, a multiple of 1/4 and below 2^20: fp32 holds every partial sum of non-negative terms exactly, in any order."""
    _, _, ref = exact_case(ks, *SHAPE, SEED)
    p = exact_params(ks)
    print(f"k = {ks}: intermediates in [{ref['lo']}, {ref['hi']}]")
    assert ref["quarter"] and ref["lo"] >= 0 and ref["hi"] < 2 ** 20
    for w in [p["ctx_w"]] + p["w"]:
        assert (w >= 0).all() and (w == np.rint(w)).all()
    for b in [p["ctx_b"]] + p["b"]:
        assert (b >= 0).all() and (b * 4 == np.rint(b * 4)).all()
    assert float(ref["ybuf"].min()) >= 0.5


@pytest.mark.parametrize("ks", [5, 3])
def test_inputs_sit_on_the_ties(ks):
    _, _, ref = exact_case(ks, *SHAPE, SEED)
    r, s = ref["resid"].ravel(), ref["scale"].ravel()
    tie = np.abs(r - np.floor(r) - 0.5) == 0
    down = tie & (np.floor(r) % 2 == 0)    # k + 1/2 with k even: rounds down to k
    up = tie & (np.floor(r) % 2 != 0)      # k odd: rounds up to k + 1
    t64 = TABLE.astype(np.float64)
    mid = (t64[:-1] + t64[1:]) / 2
    on_mid, on_entry = np.isin(s, mid), np.isin(s, t64)
    below, above = s < t64[0], s > t64[-1]
    sym = ref["sym"]
    print(f"k = {ks}: rounding ties {tie.mean():.1%} (down {down.mean():.1%}, up {up.mean():.1%}), negative residual ties "
          f"{(tie & (r < 0)).mean():.1%}; scales on a midpoint {on_mid.mean():.1%}, on an entry {on_entry.mean():.1%}, below the table "
          f"{below.mean():.1%}, above {above.mean():.2%}; symbols {sym.min()} .. {sym.max()}; table rows {ref['idx'].min()} .. {ref['idx'].max()}")
    assert tie.mean() >= 0.10 and down.any() and up.any() and (tie & (r < 0)).any() and (tie & (r > 0)).any()
    assert on_mid.mean() >= 0.10 and on_entry.any() and below.any() and above.any()
    assert np.isfinite(s).all()
    # a tie takes the FIRST minimum: the lower entry
    j = np.searchsorted(mid, s[on_mid])
    assert (ref["idx"].ravel()[on_mid] == j).all()
    assert ref["idx"].min() == 0 and ref["idx"].max() == len(TABLE) - 1


def _coded(ref):
    return np.concatenate([ref["sym"].ravel(), ref["idx"].ravel()])


@pytest.mark.parametrize("ks", [5, 3])
def test_a_wrong_window_changes_the_coded_integers(ks):
    """Power: dropping any ONE causal tap (12 for k = 5, 4 for k = 3) changes at least one coded integer, and so does reading the
    centre tap or the right neighbour (where a position not yet coded holds the latent itself)."""
    y, prior, ref = exact_case(ks, *SHAPE, SEED)
    p = exact_params(ks)
    taps = causal_taps(ks)
    assert len(taps) == (ks * ks - 1) // 2
    good = _coded(ref)
    for t in taps:
        bad = _coded(reference(p, y, prior, taps=[u for u in taps if u != t]))
        n = int((bad != good).sum())
        print(f"k = {ks}: without tap {t}: {n} coded integers differ")
        assert n > 0, t
    h = ks // 2
    for extra in [(h, h), (h, h + 1)]:
        bad = _coded(reference(p, y, prior, taps=taps + [extra], unwritten=y))
        n = int((bad != good).sum())
        print(f"k = {ks}: with tap {extra}: {n} coded integers differ")
        assert n > 0, extra
    # (the causal window itself never reads a position that is not yet coded)
    assert (_coded(reference(p, y, prior, unwritten=y)) == good).all()
