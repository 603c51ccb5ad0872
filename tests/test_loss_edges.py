"""CPU: the error budget of tests/loss_cases.py has teeth before anything runs on a card.

Six wrong implementations of the fused L1 / SSIM loss, each a short change to the numpy oracle that models one way a tiled kernel
goes wrong, must break the budget on the `noise` content at every shape where the change can be seen at all; the correct fp32
oracle passes with factor 1 (trivially: the budget is its own distance from fp64).  Whether a change can be seen is a property of
the shape alone:
  a  halo of 4 (a tap at distance 5 that crosses a multiple of 32 reads zero)      some dimension > 32
  b  replicate padding instead of zero padding                                     always
  c  a tile's last four columns take their taps one column to the left             W > 28 (a column 28..31 of some tile)
  d  the mean over the padded tile area instead of C H W                           H or W no multiple of 32
  e  the backward reads the derivative maps of channel (c + 1) % C                 C > 1
  f  an edge tile's out-of-image pixels counted in its SSIM partial                H or W no multiple of 32
MAX_EXCLUDED: at most one (shape, mutant) pair in ten may be indistinguishable.
"""
import numpy as np
import pytest

import loss_cases as lc
from oracle import loss_ref

T = lc.TILE


def _filt_halo4(a, w):
    """(a) the patch holds a halo of 4: in either pass the tap at -5 of a tile's first output and at +5 of its last reads zero."""
    C, H, W = a.shape
    # the row pass loses its two outer taps at the tile's edge columns; the column pass runs on that result
    r = np.zeros((C, H, W + 10), dtype=a.dtype)
    r[:, :, 5:5 + W] = a
    rows = sum(w[k] * r[:, :, k:k + W] for k in range(11))
    x = np.arange(W)
    rows = rows - np.where(x % T == 0, w[0] * r[:, :, 0:W], 0) - np.where(x % T == T - 1, w[10] * r[:, :, 10:10 + W], 0)
    c = np.zeros((C, H + 10, W), dtype=a.dtype)
    c[:, 5:5 + H, :] = rows
    o = sum(w[k] * c[:, k:k + H, :] for k in range(11))
    y = np.arange(H)[:, None]
    return (o - np.where(y % T == 0, w[0] * c[:, 0:H, :], 0) - np.where(y % T == T - 1, w[10] * c[:, 10:10 + H, :], 0)).astype(a.dtype)


def _filt_replicate(a, w):
    """(b) the border pixel repeated instead of zero."""
    return np.ascontiguousarray(loss_ref._filt(np.pad(a, ((0, 0), (5, 5), (5, 5)), mode="edge"), w)[:, 5:-5, 5:-5])


def _filt_shifted_group(a, w):
    """(c) columns 28..31 of every tile hold the result of the column to their left."""
    o = loss_ref._filt(a, w)
    x = np.arange(a.shape[2])
    last = x[x % T >= T - 4]
    o[:, :, last] = o[:, :, last - 1].copy()
    return o


def _padded_area(shape):
    C, H, W = shape
    return C * (-(-H // T) * T) * (-(-W // T) * T)


def _mutant(name, img, gt):
    """The fp32 outputs of mutant `name`."""
    f32 = np.float32
    if name in "abc":
        return lc.outputs(img, gt, f32, filt={"a": _filt_halo4, "b": _filt_replicate, "c": _filt_shifted_group}[name])
    o = lc.outputs(img, gt, f32)
    if name == "d":
        s = f32(img.size) / f32(_padded_area(img.shape))
        o["g_l1"], o["g_ssim"], o["l1"], o["ssim_mean"] = o["g_l1"] * s, o["g_ssim"] * s, o["l1"] * float(s), o["ssim_mean"] * float(s)
    elif name == "e":
        o["g_l1"], o["g_ssim"] = loss_ref.l1_ssim_grads(img, gt, *(np.roll(o[q], -1, axis=0) for q in lc.MAPS), f32)
    elif name == "f":
        C, H, W = img.shape
        pad = ((0, 0), (0, -H % T), (0, -W % T))
        o["tile_ssim"] = loss_ref.l1_ssim_terms(np.pad(img, pad), np.pad(gt, pad), f32, T)["tile_ssim"]
        o["ssim_mean"] = float(o["tile_ssim"].sum(dtype=np.float64)) / img.size
    o["grad"] = lc.combine(o, *lc.G_DEFAULT)
    return o


MUTANTS = {
    "a": lambda C, H, W: H > T or W > T,
    "b": lambda C, H, W: True,
    "c": lambda C, H, W: W > T - 4,
    "d": lambda C, H, W: H % T != 0 or W % T != 0,
    "e": lambda C, H, W: C > 1,
    "f": lambda C, H, W: H % T != 0 or W % T != 0,
}
MAX_EXCLUDED = 0.1


def test_shapes_cover_every_size_and_channel_count():
    for v in lc.SIZES:
        assert any(s[1] == v for s in lc.SHAPES) and any(s[2] == v for s in lc.SHAPES), v
    assert {s[0] for s in lc.SHAPES} == {1, 2, 3, 4}
    assert (1, 1, 1) in lc.SHAPES
    assert any(s != (1, 1, 1) and s[1] <= 5 and s[2] <= 5 for s in lc.SHAPES) and any(s[1] >= 33 and s[2] >= 33 for s in lc.SHAPES)
    assert len(lc.SHAPES) == len(set(lc.SHAPES)) <= 26
    assert [s for s, c in lc.CASES if c == "noise"] == lc.SHAPES
    for c in lc.CLASSES[1:]:
        assert [s for s, k in lc.CASES if k == c] == lc.CLASS_SHAPES


def test_at_most_one_pair_in_ten_is_declared_indistinguishable():
    pairs = [(s, m) for s in lc.SHAPES for m in MUTANTS]
    out = [(s, m) for s, m in pairs if not MUTANTS[m](*s)]
    for m in MUTANTS:
        print(f"[loss-edges] mutant {m}: {sum(1 for _, k in out if k == m)} of {len(lc.SHAPES)} shapes excluded")
    print(f"[loss-edges] excluded {len(out)} of {len(pairs)}")
    assert len(out) <= MAX_EXCLUDED * len(pairs), (len(out), len(pairs))


@pytest.mark.parametrize("case", lc.NOISE_CASES, ids=lc.case_id)
@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_breaks_the_budget_wherever_it_can_be_seen(name, case):
    shape, cls = case
    ref = lc.reference(shape, cls)
    r = ref.ratios(_mutant(name, ref.img, ref.gt))
    worst = max(r.values())
    print(f"[loss-edges] mutant {name} {lc.case_id(case)}: {r}")
    if MUTANTS[name](*shape):
        assert worst > 1.0, (name, shape, r)
    else:       # the predicate is honest: where it says "cannot be seen" the mutant is the correct code to within the budget
        assert worst <= 1.0, (name, shape, r)


@pytest.mark.parametrize("case", lc.CASES + lc.BIG_CASES, ids=lc.case_id)
def test_correct_fp32_oracle_passes_with_factor_one(case):
    ref = lc.reference(*case)
    r = ref.ratios(ref.o32, factor=1.0)
    for g in lc.G_PAIRS:
        r[f"grad{g}"] = ref.ratio(g, lc.combine(ref.o32, *g), factor=1.0)
    assert max(r.values()) <= 1.0, r
    for q in ("ssim", "grad") + lc.MAPS:
        assert np.isfinite(ref.o32[q]).all() and np.isfinite(ref.o64[q]).all(), q


@pytest.mark.parametrize("case", lc.CASES + lc.BIG_CASES, ids=lc.case_id)
def test_tile_sums_add_up_to_the_means(case):
    ref = lc.reference(*case)
    l1, s, g_l1, g_s = loss_ref.l1_ssim(ref.img, ref.gt, dtype=np.float64)
    n = ref.img.size
    C, H, W = ref.shape
    assert ref.o64["tile_l1"].shape == ref.o64["tile_ssim"].shape == (C, -(-H // T), -(-W // T))
    assert abs(ref.o64["tile_l1"].sum() / n - l1) <= 1e-12 * abs(l1)
    assert abs(ref.o64["tile_ssim"].sum() / n - s) <= 1e-12 * abs(s)
    assert np.array_equal(g_l1, ref.o64["g_l1"]) and np.array_equal(g_s, ref.o64["g_ssim"])
    # another tile size, and a rectangular one, cut the same sum
    t = loss_ref.l1_ssim_terms(ref.img, ref.gt, np.float64, (16, 8))
    assert t["tile_ssim"].shape == (C, -(-H // 16), -(-W // 8))
    assert abs(t["tile_ssim"].sum() / n - s) <= 1e-12 * abs(s) and abs(t["tile_l1"].sum() / n - l1) <= 1e-12 * abs(l1)


def test_contents_are_what_they_claim():
    for shape in lc.CLASS_SHAPES:
        img, gt = lc.images(shape, "same")
        assert np.array_equal(img, gt)
        img, gt = lc.images(shape, "eq_px")
        eq = (img == gt).reshape(-1)
        assert eq[::3].all() and (img.size < 3 or not eq.all())
        img, gt = lc.images(shape, "hdr")
        assert gt.max() <= 8.0 and (img.size < 100 or gt.max() > 4.0)
        img, gt = lc.images(shape, "black")
        assert not gt.any() and set(np.unique(img)) <= {np.float32(0.0), np.float32(1e-3)}
        again = lc.images(shape, "noise")
        assert np.array_equal(again[0], lc.images(shape, "noise")[0])


def test_report_E_table():
    """Prints E per case and quantity (pytest -s): the table of the pull request's summary."""
    rows = []
    for case in lc.CASES + lc.BIG_CASES:
        ref = lc.reference(*case)
        gmax = float(np.abs(lc.combine(ref.o64, *lc.G_DEFAULT)).max())
        rows.append((lc.case_id(case), ref.E("ssim"), ref.E("dmu1"), ref.E("ds1"), ref.E("ds12"), ref.E(lc.G_DEFAULT),
                     ref.E(lc.G_DEFAULT) / gmax if gmax else 0.0, abs(ref.o32["ssim_mean"] - ref.o64["ssim_mean"])))
    print("\n[loss-E] case | E ssim | E dmu1 | E ds1 | E ds12 | E grad | E grad / max|grad| | |s32 - s64|")
    for r in rows:
        print("[loss-E] " + " | ".join([r[0]] + [f"{v:.2e}" for v in r[1:]]))
    assert all(np.isfinite(r[1:]).all() for r in rows)
