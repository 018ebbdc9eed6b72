"""The yardstick of the activation and softmax sites (tests/activation_reference.py) against the CPU oracle: on the whole edge grid
the C oracle ALONE -- without the anchor term of the bound -- stays inside the per-element bound, for every kind, with the default
and the non-default attributes, for swish at three beta and for the softmax rows; and the region in which the oracle's swish reverse
factor is NaN is pinned.  No GPU."""
import numpy as np
import pytest

import activation_reference as ar


def _worst(got, ref, t):
    f, scale, a = ref
    sh = ar.share(got, f, scale, a, t)
    assert not np.isnan(sh).any()
    return float(sh.max())


def test_grid_holds_the_edges_it_names():
    t = ar.edge_grid()
    assert t.dtype == np.float32 and t.size == 2 * 4096 + 2 * len(ar.EDGE_VALUES) + 6 * len(ar.THRESHOLDS)
    assert np.isfinite(t).all() and np.abs(t).max() == 104.0
    assert (np.signbit(t) & (t == 0)).any() and (~np.signbit(t) & (t == 0)).any(), "both zeros"
    for th in (0.25, -0.5, 1.0, 0.3):
        th = np.float32(th)
        for v in (th, np.nextafter(th, np.float32(np.inf)), np.nextafter(th, np.float32(-np.inf))):
            assert (t == v).any(), f"{v!r} missing"
    assert (np.abs(t) == np.float32(1e-40)).sum() == 2, "subnormal inputs"
    e = ar.edge_grid(exact_div=True)
    assert e.shape == t.shape and (e.view(np.int32) & 7 == 0).all()
    for d in (1, 2, 3, 4):
        assert np.array_equal((np.float32(d) * e).astype(np.float64), d * e.astype(np.float64)), "d * t is exact"
        assert np.array_equal((np.float32(d) * e) / np.float32(d), e)


@pytest.mark.parametrize("kind", ["none", "relu", "sigmoid", "tanh"])
def test_plain_oracle_alone_is_inside_the_bound(oracle, kind):
    t = ar.edge_grid()
    w = _worst(oracle.activation(kind, t), ar.forward(kind, t), t)
    print(f"{kind}: oracle alone {w:.3f} of the bound")
    assert w < 1.0


@pytest.mark.parametrize("name,attrs", ar.attributed_cases())
def test_attributed_oracle_alone_is_inside_the_bound(oracle, name, attrs):
    t = ar.edge_grid()
    g = np.random.default_rng(3).standard_normal(t.size).astype(np.float32)
    scale, p0, p1 = ar.resolve(name, attrs)
    w = _worst(oracle.activation_param(name, t, scale, p0, p1), ar.forward(name, t, scale, p0, p1), t)
    wb = _worst(oracle.activation_param_bwd(name, t, g, scale, p0, p1), ar.reverse(name, t, g, scale, p0, p1), t)
    print(f"{name} {attrs}: oracle alone {w:.3f} forward, {wb:.3f} reverse, of the bound")
    assert w < 1.0 and wb < 1.0
    if name not in ar.TRANSCENDENTAL:                 # no transcendental: the float64 form rounds to the oracle's value
        assert w <= 0.02 and wb <= 0.02


@pytest.mark.parametrize("beta", ar.SWISH_BETAS)
def test_swish_oracle_alone_is_inside_the_bound(oracle, beta):
    t = ar.edge_grid()
    g = ar.swish_upstream(t.size)
    w = _worst(oracle.swish(t, beta), ar.forward("swish", t, beta=beta), t)
    d = oracle.swish_bwd(t, g, beta)
    bx = np.float32(beta) * t
    nan = np.isnan(d)
    assert not nan[bx <= ar.SWISH_FINITE].any() and nan[bx >= 45.0].all() and not (d[bx > ar.SWISH_FINITE] == 0).any()
    fin = bx <= ar.SWISH_FINITE                          # above, the fp32 formula overflows: that region is pinned by its NaN mask
    assert np.isfinite(d[fin]).all()
    ref = ar.reverse("swish", t, g, beta=beta)
    wb = _worst(d[fin], tuple(r[fin] for r in ref), t[fin])
    print(f"swish beta {beta}: oracle alone {w:.3f} forward, {wb:.3f} reverse, of the bound")
    assert w < 1.0 and wb < 1.0


def test_swish_reverse_factor_is_nan_from_beta_x_45_on(oracle):
    """(e + 1)^2 and e (beta x + e + 1) overflow together once e^2 passes FLT_MAX, at beta x = 44.36...: the factor is inf / inf
    from there on, not from beta x ~ 88 (where e itself overflows)"""
    one = np.ones(1, np.float32)
    for beta in ar.SWISH_BETAS:
        for bx, want_nan in ((-104.0, False), (0.0, False), (32.0, False), (44.0, False), (45.0, True), (64.0, True), (88.0, True), (104.0, True)):
            x = np.asarray([bx / beta], np.float32)
            assert np.float32(beta) * x[0] == np.float32(bx)
            d = oracle.swish_bwd(x, one, beta)[0]
            assert np.isnan(d) == want_nan, f"beta {beta}, beta x = {bx}: {d!r}"
            if not want_nan:
                assert np.isfinite(d)
    below = np.nextafter(np.float32(0.5 * np.log(float(np.finfo(np.float32).max))), np.float32(0))
    assert np.isfinite(oracle.swish_bwd(np.asarray([below - np.float32(1e-3)]), one, 1.0)[0])


@pytest.mark.parametrize("F", ar.SOFTMAX_F)
def test_softmax_oracle_alone_is_inside_the_bound(oracle, F):
    z = ar.softmax_rows(F)
    assert z.shape == (70, F) and z.dtype == np.float32
    assert np.array_equal(z, ar.softmax_rows(F)), "seeded"
    y = oracle.softmax_cols(z)
    w = _worst(y, ar.softmax(z), z)
    g = np.random.default_rng(F).standard_normal(z.shape).astype(np.float32)
    wb = _worst(oracle.softmax_cols_bwd(y, g), ar.softmax_reverse(y, g), z)
    print(f"softmax F = {F}: oracle alone {w:.3f} forward, {wb:.3f} reverse, of the bound")
    assert w < 1.0 and wb < 1.0
    assert np.isfinite(y).all() and (y >= 0).all() and (y <= 1).all()
    assert (np.abs(y.astype(np.float64).sum(1) - 1.0) <= F * 2.0 ** -23).all()
    lead = np.sort(z.astype(np.float64), axis=1)
    if F > 1:
        gaps = lead[:63, -1] - lead[:63, -2]
        for k, spread in enumerate(ar.SPREADS):
            assert (gaps[9 * k:9 * k + 9] >= spread * (1 - 1e-6) - 2e-3 * (spread > 0)).all()
        assert F < 3 or ((z[63:] == 0).sum(1) >= 3).all(), "three-way ties"


def test_assert_each_names_the_worst_element():
    t = np.asarray([0.5, -3.0, 20.0], np.float32)
    f, scale, a = ar.forward("sigmoid", t)
    good = f.astype(np.float32)
    assert ar.assert_each(good, good, f, scale, a, t, "sigmoid") <= 1.0
    off = good.copy()
    off[1] *= np.float32(1 + 5e-5)
    with pytest.raises(AssertionError, match=r"worst at \(1,\): t = -3\.0, .* 4\.99 of its bound"):
        ar.assert_each(off, good, f, scale, a, t, "sigmoid")
    off = good.copy()
    off[2] = np.nan
    with pytest.raises(AssertionError, match="outside the bound"):
        ar.assert_each(off, good, f, scale, a, t, "sigmoid")
    # an output 50 % off that the tensor's maximum hides from a max-norm
    small = ar.forward("sigmoid", np.asarray([-30.0, 5.0], np.float32))
    off = small[0].astype(np.float32)
    off[0] *= np.float32(0.5)
    with pytest.raises(AssertionError):
        ar.assert_each(off, small[0].astype(np.float32), *small, np.asarray([-30.0, 5.0], np.float32), "sigmoid")
