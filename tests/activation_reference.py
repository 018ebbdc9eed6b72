"""float64 forms of every activation, its reverse factor and the softmax, written from the formulas of oracle/athena_oracle.c, the
pre-activations at which such functions go wrong (edge_grid, softmax_rows), and the per-element bound they are held to (assert_each).
numpy only.

Every form returns (value, scale, a):
  value  the float64 result; attributes are taken as their fp32 roundings, the softmax is taken over the fp32 logits
  scale  the magnitude of the form's own terms, the quantity an fp32 evaluation's error is relative to.  It is |value| except where
         the formula cancels: selu's negative branch (expf(x) - 1), the sigmoid / tanh reverse factors (1 - y, 1 - y*y), the swish
         reverse factor and the softmax reverse (y g - y dot)
  a      the argument the form passes to exp (0 where it has none).  One rounding of that argument moves exp by |a| 2^-24 relative;
         a route that forms it as x * fl(-log2(e) * fl(1/d)) for the hardware exp2 rounds about 2.5 times, which is 4e-6 at
         |a| = 32 and 1e-5 at |a| = 80.  The bound therefore grows as max(1, |a| / 32), which leaves about 2.5 x room at every |a|

The bound of assert_each:   |dev - f64| <= |oracle32 - f64| + 1e-5 scale max(1, |a|/32) + FLT_MIN max(1, |t|)
1e-5 is the project's bound; the last term covers results that the hardware exp / rcp flush to zero."""
import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)
RTOL = 1e-5

# name -> ((first attribute, default), (second attribute, default)): the reference's reset_* values, as in athena_amd.ops.ACTP
DEFAULTS = {"linear": (), "none": (), "relu": (("threshold", 0.0),), "sigmoid": (), "tanh": (), "leaky_relu": (("alpha", 0.01),),
            "selu": (("alpha", 1.67326), ("lambda", 1.0507)), "gaussian": (("sigma", 1.5), ("mu", 0.0)),
            "piecewise": (("gradient", 0.1), ("limit", 1.0))}
TRANSCENDENTAL = ("sigmoid", "tanh", "selu", "gaussian", "swish")
SWISH_BETAS = (0.5, 1.0, 2.0)


def resolve(name, attrs):
    """(scale, p0, p1) as the oracle's attributed entries take them; scale applies only when it differs from 1 by more than 1e-6
    (apply_scaling)"""
    attrs = dict(attrs)
    scale = float(attrs.pop("scale", 1.0))
    if not abs(np.float32(scale) - np.float32(1)) > np.float32(1e-6):
        scale = 1.0
    p = [0.0, 0.0]
    for k, (key, default) in enumerate(DEFAULTS[name]):
        p[k] = float(attrs.pop(key, default))
    assert not attrs, f"{name} has no attribute(s) {sorted(attrs)}"
    return scale, p[0], p[1]


def attributed_cases():
    """ATTRIBUTED of tests/test_gpu_network.py (the non-default attributes, and the defaults of the kinds that have attributes) plus
    the defaults of the four kinds it lists with attributes only"""
    from test_gpu_network import ATTRIBUTED

    return list(ATTRIBUTED) + [(k, {}) for k in ("relu", "linear", "sigmoid", "tanh")]


def _r(v):
    return np.float64(np.float32(v))


def _x(t):
    t = np.asarray(t)
    assert t.dtype == np.float32, "pre-activations are fp32"
    return t.astype(np.float64)


# ---- forward ------------------------------------------------------------------------------------------------------------------------
def forward(kind, t, scale=1.0, p0=0.0, p1=0.0, beta=1.0):
    """y = f(t) * scale (oracle_activation, oracle_activation_param, oracle_swish)"""
    x, s, p0, p1, beta = _x(t), _r(scale), _r(p0), _r(p1), _r(beta)
    a = np.zeros_like(x)
    mag = None
    with np.errstate(over="ignore", under="ignore"):
        if kind in ("none", "linear"):
            f = x
        elif kind == "relu":
            f = np.where(x > p0, x, p0)
        elif kind == "sigmoid":
            a = -x
            f = 1.0 / (1.0 + np.exp(a))
        elif kind == "tanh":
            f = np.tanh(x)
        elif kind == "leaky_relu":
            f = np.where(x * p0 > x, x * p0, x)
        elif kind == "selu":
            neg = ~(x > 0.0)
            e = np.exp(np.where(neg, x, 0.0))
            f = np.where(neg, (e - 1.0) * p0 * p1, x * p1)
            mag = np.where(neg, (e + 1.0) * abs(p0 * p1), np.abs(f))
            a = np.where(neg, x, 0.0)
        elif kind == "gaussian":
            u = (x - p1) / p0
            a = -0.5 * u * u
            f = 1.0 / (np.sqrt(2.0 * np.pi) * p0) * np.exp(a)
        elif kind == "piecewise":
            f = np.where(x >= p1, p0 * (x - p1) + p1, np.where(x <= -p1, p0 * (x + p1) - p1, x))
        elif kind == "swish":
            a = -beta * x
            f = x * (1.0 / (1.0 + np.exp(a)))
        else:
            raise ValueError(kind)
    f = f * s
    return f, (np.abs(f) if mag is None else mag * abs(s)), a


# ---- reverse factors, differentiated at the INPUT ------------------------------------------------------------------------------------
def reverse(kind, t, g, scale=1.0, p0=0.0, p1=0.0, beta=1.0):
    """d = f'(t) * (g * scale) (oracle_activation_param_bwd, oracle_swish_bwd)"""
    x, s, p0, p1, beta = _x(t), _r(scale), _r(p0), _r(p1), _r(beta)
    u = _x(g) * s
    a = np.zeros_like(x)
    mag = None
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if kind in ("none", "linear"):
            d = u
        elif kind == "relu":
            d = np.where(x > p0, u, 0.0)
        elif kind == "sigmoid":
            a = -x
            y = 1.0 / (1.0 + np.exp(a))
            d = u * y * (1.0 - y)
            mag = np.abs(u) * y * (1.0 + y)
        elif kind == "tanh":
            y = np.tanh(x)
            d = u * (1.0 - y * y)
            mag = np.abs(u) * (1.0 + y * y)
        elif kind == "leaky_relu":
            d = np.where(x * p0 > x, u * p0, u)
        elif kind == "selu":
            neg = ~(x > 0.0)
            d = np.where(neg, u * (np.exp(np.where(neg, x, 0.0)) * p0 * p1), u * p1)
            a = np.where(neg, x, 0.0)
        elif kind == "gaussian":
            w = (x - p1) / p0
            a = -0.5 * w * w
            f = 1.0 / (np.sqrt(2.0 * np.pi) * p0) * np.exp(a)
            d = u * (-(x - p1) / (p0 * p0) * f)
        elif kind == "piecewise":            # get_partial_piecewise_val as written: always true for limit >= 0
            d = np.where((x <= p1) | (x >= -p1), u, u * p0)
        elif kind == "swish":
            bx = beta * x
            a = -bx
            e = np.exp(bx)
            d = u * e * (bx + e + 1.0) / ((e + 1.0) * (e + 1.0))
            mag = np.abs(u) * e * (np.abs(bx) + e + 1.0) / ((e + 1.0) * (e + 1.0))
        else:
            raise ValueError(kind)
    return d, (np.abs(d) if mag is None else mag), a


SWISH_FINITE = 44.0     # beta x up to which the fp32 reverse factor is finite for |g| <= 1.5; it is NaN from 45 on


def swish_upstream(n):
    """upstream gradients of magnitude 1 .. 1.5: the numerator g e (beta x + e + 1) then overflows no later than (e + 1)^2 does, so
    that past the overflow the factor is inf or NaN (inf / inf), never a finite / inf = 0 that depends on g"""
    rng = np.random.default_rng(4)
    return (rng.uniform(1.0, 1.5, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


# ---- softmax over the features of each row -------------------------------------------------------------------------------------------
def softmax(z):
    """(y, scale = y, a = z - max) over the fp32 logits z [N, F]"""
    x = _x(z)
    a = x - x.max(axis=1, keepdims=True)
    with np.errstate(under="ignore"):
        e = np.exp(a)
    y = e / e.sum(axis=1, keepdims=True)
    return y, y, a


def softmax_reverse(y, g):
    """dz = y g - y sum(y g) from the given fp32 y (the device's own); scale = |y g| + |y| sum|y g|"""
    y, g = _x(y), _x(g)
    yg = y * g
    return yg - y * yg.sum(axis=1, keepdims=True), np.abs(yg) + np.abs(y) * np.abs(yg).sum(axis=1, keepdims=True), np.zeros_like(y)


# ---- the grid ------------------------------------------------------------------------------------------------------------------------
EDGE_VALUES = (0.0, 1e-40, 1e-30, 1e-3, 0.5, 1.0, 2.0, 5.0, 8.3, 16.0, 17.0, 32.0, 44.0, 45.0, 64.0, 87.0, 88.5, 88.8, 89.0, 100.0, 104.0)
# relu at 0 and at `threshold`, leaky relu and selu at 0, piecewise at +-`limit`, the gaussian's mu -- defaults and the non-default
# attributes of ATTRIBUTED
THRESHOLDS = (0.0, 0.25, 0.5, 1.0, 0.3)


def clear_low_bits(t, bits=3):
    """the fp32 values with their low mantissa bits cleared: d * t is then exact for d <= 2^bits / 2"""
    return (np.ascontiguousarray(t, np.float32).view(np.int32) & np.int32(~((1 << bits) - 1))).view(np.float32)


def edge_grid(exact_div=False):
    """fp32 pre-activations [n]: the saturation / overflow / subnormal points +-EDGE_VALUES (both zeros), every threshold with the
    float on either side of it, then 4096 magnitudes log-uniform in [1e-6, 32], each with both signs"""
    rng = np.random.default_rng(20240)
    m = np.exp(rng.uniform(np.log(1e-6), np.log(32.0), 4096)).astype(np.float32)
    e = np.asarray(EDGE_VALUES, np.float32)
    th = np.asarray(THRESHOLDS, np.float32)
    th = np.concatenate([th, -th])
    near = np.concatenate([np.nextafter(th, np.float32(np.inf)), np.nextafter(th, np.float32(-np.inf))]).astype(np.float32)
    t = np.concatenate([e, -e, th, near, np.stack([m, -m], axis=1).ravel()]).astype(np.float32)
    return clear_low_bits(t) if exact_div else t


N_EDGES = 2 * len(EDGE_VALUES) + 6 * len(THRESHOLDS)        # the grid's leading values: what a tensor smaller than the grid keeps


def planted(shape, exact_div=False):
    """a tensor of this shape filled with the grid, repeated; one smaller than the grid keeps the edges and thresholds and as many
    of the magnitudes, with both signs, as fit"""
    n = int(np.prod(shape))
    assert n >= N_EDGES + 512
    return np.resize(edge_grid(exact_div), n).reshape(shape)


# ---- softmax rows --------------------------------------------------------------------------------------------------------------------
SOFTMAX_F = (1, 2, 4, 8, 9, 16, 17, 48, 49, 64, 65, 128, 130, 200)      # both sides of every G switch (F <= 8, <= 48)
SPREADS = (0.0, 1.0, 10.0, 32.0, 64.0, 100.0, 1e4)
OFFSETS = (0.0, 1e4, -1e4)


def softmax_rows(F, seed=0):
    """fp32 logits [70, F]: spread x offset x place of the maximum (index 0, F - 1, a random one), then one row per spread whose
    maximum is tied three times.  The largest logit is `offset`; every other one lies `spread` to 2 `spread` below it (all equal
    at spread 0)"""
    rng = np.random.default_rng(1000 * F + seed)
    rows = []
    for spread in SPREADS:
        for off in OFFSETS:
            for place in (0, F - 1, int(rng.integers(0, F))):
                r = (np.float32(off) + (-spread * (1.0 + rng.uniform(0, 1, F))).astype(np.float32)).astype(np.float32)
                r[place] = np.float32(off)
                rows.append(r)
    for spread in SPREADS:
        r = (-spread * (1.0 + rng.uniform(0, 1, F))).astype(np.float32)
        r[rng.choice(F, min(3, F), replace=False)] = 0.0
        rows.append(r)
    return np.stack(rows).astype(np.float32)


# ---- the bound -----------------------------------------------------------------------------------------------------------------------
def bound(scale, a, t):
    scale, a, t = (np.asarray(v, np.float64) for v in (scale, a, t))
    return RTOL * np.abs(scale) * np.maximum(1.0, np.abs(a) / 32.0) + FLT_MIN * np.maximum(1.0, np.abs(t))


def share(got, f64, scale, a, t, anchor=None):
    """|got - f64| over the bound, element by element; anchor: the fp32 oracle, whose own distance from f64 is added to the bound"""
    got, f64 = np.asarray(got, np.float64), np.asarray(f64, np.float64)
    b = np.broadcast_to(bound(scale, a, t), f64.shape).copy()
    if anchor is not None:
        b += np.abs(np.asarray(anchor, np.float64) - f64)
    with np.errstate(invalid="ignore"):
        return np.abs(got - f64) / b


def assert_each(dev, oracle32, f64, scale, a, t, what):
    """the per-element form of helpers.assert_close; returns the worst share of the bound"""
    dev = np.asarray(dev)
    assert dev.shape == np.shape(f64), f"{what}: shape {dev.shape} != {np.shape(f64)}"
    sh = share(dev, f64, scale, a, t, anchor=oracle32)
    bad = ~(sh <= 1.0)                                  # a NaN on either side is a failure
    if bad.any():
        k = tuple(int(i) for i in np.unravel_index(int(np.argmax(np.where(np.isnan(sh), np.inf, sh))), sh.shape))
        tt = np.broadcast_to(np.asarray(t), sh.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {sh.size} element(s) outside the bound; worst at {k}: t = {float(tt[k])!r}, "
                             f"device {float(dev[k])!r}, oracle {float(np.asarray(oracle32)[k])!r}, float64 {float(np.asarray(f64)[k])!r}, "
                             f"{float(sh[k]):.3g} of its bound")
    worst = float(sh.max()) if sh.size else 0.0
    print(f"{what}: worst share of the bound {worst:.3f}")
    return worst
