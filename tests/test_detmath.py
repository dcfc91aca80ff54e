"""acn_detmath.h (the arithmetic contract shared by oracle and GPU) against glibc's libm, on the CPU."""
import numpy as np

OPS = {"sin": 0, "cos": 1, "tan": 2, "acos": 3, "log": 4, "exp": 5, "pow": 6, "sqrt": 7, "div": 8, "u64_to_f64": 9,
       "frexp_mant": 10, "asin": 11, "atan": 12, "atan2": 13, "llrint": 14}


def cpu_eval(lib, op, x, y=None):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    yp = None
    if y is not None:
        y = np.ascontiguousarray(y, dtype=np.float64)
        yp = y.ctypes.data
    lib.detmath_eval(OPS[op], x.ctypes.data, yp, out.ctypes.data, x.size)
    return out


def ulp_err(got, ref):
    return np.abs(got - ref) / np.spacing(np.abs(ref))


def test_sin_cos_tan(detmath_cpu):
    rng = np.random.default_rng(1)
    x = rng.uniform(0, 2 * np.pi, 400000)
    s, c = np.sin(x), np.cos(x)
    ok = np.abs(s) > 1e-3
    assert ulp_err(cpu_eval(detmath_cpu, "sin", x)[ok], s[ok]).max() <= 1.0
    ok = np.abs(c) > 1e-3
    assert ulp_err(cpu_eval(detmath_cpu, "cos", x)[ok], c[ok]).max() <= 1.0
    # near the zeros the kernels stay absolutely accurate
    assert np.abs(cpu_eval(detmath_cpu, "sin", x) - s).max() < 2.3e-16
    assert np.abs(cpu_eval(detmath_cpu, "cos", x) - c).max() < 2.3e-16
    xt = rng.uniform(0, np.pi, 400000)
    ok = np.abs(np.cos(xt)) > 1e-3
    assert ulp_err(cpu_eval(detmath_cpu, "tan", xt)[ok], np.tan(xt)[ok]).max() <= 2.0
    # odd / even symmetry
    assert np.array_equal(cpu_eval(detmath_cpu, "sin", -x), -cpu_eval(detmath_cpu, "sin", x))
    assert np.array_equal(cpu_eval(detmath_cpu, "cos", -x), cpu_eval(detmath_cpu, "cos", x))


def test_acos_log_exp(detmath_cpu):
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, 400000)
    assert ulp_err(cpu_eval(detmath_cpu, "acos", x), np.arccos(x)).max() <= 1.0
    assert cpu_eval(detmath_cpu, "acos", np.array([1.0]))[0] == 0.0
    assert cpu_eval(detmath_cpu, "acos", np.array([-1.0]))[0] == np.pi
    assert np.isnan(cpu_eval(detmath_cpu, "acos", np.array([1.0000000000000002]))[0])
    xl = np.exp(rng.uniform(-12, 12, 400000))
    assert ulp_err(cpu_eval(detmath_cpu, "log", xl), np.log(xl)).max() <= 1.0
    assert cpu_eval(detmath_cpu, "log", np.array([1.0]))[0] == 0.0
    assert cpu_eval(detmath_cpu, "log", np.array([0.0]))[0] == -np.inf
    xe = rng.uniform(-40, 40, 400000)
    assert ulp_err(cpu_eval(detmath_cpu, "exp", xe), np.exp(xe)).max() <= 1.0
    assert cpu_eval(detmath_cpu, "exp", np.array([800.0]))[0] == np.inf
    assert cpu_eval(detmath_cpu, "exp", np.array([-800.0]))[0] == 0.0


def test_pow_colour_semantics(detmath_cpu):
    rng = np.random.default_rng(3)
    x = rng.uniform(0, 1, 200000)
    y = rng.uniform(0, 6, 200000)
    got = cpu_eval(detmath_cpu, "pow", x, y)
    ref = np.power(x, y)
    assert (np.abs(got - ref) <= 1e-13 * ref + 1e-300).all()
    # exact identities the renderer relies on: gamma == 1 must not move a colour, black stays black
    assert np.array_equal(cpu_eval(detmath_cpu, "pow", x, np.ones_like(x)), x)
    assert np.array_equal(cpu_eval(detmath_cpu, "pow", np.zeros(4), np.array([0.7, 0.9, 1.0, 2.0])), np.zeros(4))
    assert cpu_eval(detmath_cpu, "pow", np.array([1e40]), np.array([0.9]))[0] > 1.0


def test_frexp_and_conversion(detmath_cpu):
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.normal(size=100000) * 10.0 ** rng.integers(-300, 300, 100000), [0.0, -0.0, 5e-324, -5e-324]])
    m, _ = np.frexp(x)
    assert np.array_equal(cpu_eval(detmath_cpu, "frexp_mant", x), m)
    u = rng.integers(0, 2 ** 63, 100000, dtype=np.uint64) * 2 + rng.integers(0, 2, 100000, dtype=np.uint64)
    got = cpu_eval(detmath_cpu, "u64_to_f64", u.view(np.float64))
    assert np.array_equal(got, u.astype(np.float64))


def _mp_ulp_err(got, fn, *args):
    """|got - f( args )| in ulps of the exact value, f evaluated by mpmath at 80 digits"""
    import mpmath
    mpmath.mp.dps = 80
    worst = 0.0
    for g, *a in zip(got, *args):
        ref = fn(*[mpmath.mpf(float(v)) for v in a])
        ulp = np.spacing(abs(float(ref))) if ref != 0 else 5e-324
        worst = max(worst, float(abs(mpmath.mpf(float(g)) - ref) / mpmath.mpf(float(ulp))))
    return worst


def test_asin_atan(detmath_cpu):
    """the sphere's texture projection (acn_device.h: obj_color_dev): asin and atan at the <= 1 ulp DESIGN.md section 2 states"""
    import mpmath
    rng = np.random.default_rng(5)
    # every branch of acn_asin: |x| < 2^-27, < 0.5, < 0.975, up to 1; the branch points and their neighbours
    edges = np.array([0.0, -0.0, 2.0 ** -27, 0.5, 0.975, 1.0, 2.0 ** -1022, 5e-324])
    edges = np.concatenate([edges, np.nextafter(edges, 2.0), np.nextafter(edges, -2.0)])
    edges = edges[np.abs(edges) <= 1.0]
    x = np.concatenate([rng.uniform(-1, 1, 400000), 1.0 - np.exp(rng.uniform(-36, 0, 50000)), np.exp(rng.uniform(-40, 0, 50000)), edges, -edges])
    got = cpu_eval(detmath_cpu, "asin", x)
    assert ulp_err(got, np.arcsin(x)).max() <= 1.0
    assert _mp_ulp_err(got[:2000], mpmath.asin, x[:2000]) <= 1.0 and _mp_ulp_err(got[-4 * edges.size:], mpmath.asin, x[-4 * edges.size:]) <= 1.0
    assert np.array_equal(cpu_eval(detmath_cpu, "asin", -x).view(np.uint64), (-got).view(np.uint64))          # odd, -0 included
    assert np.array_equal(cpu_eval(detmath_cpu, "asin", np.array([1.0, -1.0])), np.array([np.pi / 2, -np.pi / 2]))
    z = cpu_eval(detmath_cpu, "asin", np.array([0.0, -0.0]))
    assert np.array_equal(z, [0.0, 0.0]) and np.array_equal(np.signbit(z), [False, True])
    assert np.isnan(cpu_eval(detmath_cpu, "asin", np.array([1.0000000000000002, -1.0000000000000002, np.inf, np.nan]))).all()
    # every range of acn_atan: 2^-29, 7/16, 11/16, 19/16, 39/16, 2^66
    edges = np.array([0.0, 2.0 ** -29, 0.4375, 0.6875, 1.0, 1.1875, 2.4375, 2.0 ** 66, 1e300, np.inf])
    edges = np.concatenate([edges, np.nextafter(edges, np.inf), np.nextafter(edges, -1.0)])
    xa = np.concatenate([rng.normal(size=300000) * np.exp(rng.uniform(-30, 50, 300000)), rng.uniform(-3, 3, 200000), edges, -edges])
    got = cpu_eval(detmath_cpu, "atan", xa)
    assert ulp_err(got, np.arctan(xa)).max() <= 1.0
    assert _mp_ulp_err(got[:2000], mpmath.atan, xa[:2000]) <= 1.0 and _mp_ulp_err(got[-2 * edges.size:], mpmath.atan, xa[-2 * edges.size:]) <= 1.0
    assert np.array_equal(cpu_eval(detmath_cpu, "atan", -xa).view(np.uint64), (-got).view(np.uint64))
    assert np.array_equal(cpu_eval(detmath_cpu, "atan", np.array([np.inf, -np.inf])), np.array([np.pi / 2, -np.pi / 2]))
    assert np.isnan(cpu_eval(detmath_cpu, "atan", np.array([np.nan]))[0])


def test_atan2(detmath_cpu):
    """acn_atan2( y, x ): the four quadrants, the axes, the signed zeros and the infinities as C99 Annex F has them.  The bound is the
    contract's: the distance to glibc.  (Against the exact value the second and third quadrant, pi - ( z - pi_lo ) after a rounded
    quotient, reach 1.2 ulp -- measured with mpmath on these operands -- where glibc stays below 0.6.)"""
    rng = np.random.default_rng(6)
    n = 400000
    y = rng.normal(size=n) * np.exp(rng.uniform(-20, 20, n))
    x = rng.normal(size=n) * np.exp(rng.uniform(-20, 20, n))
    x[:1000] = 1.0                                          # the x == 1 shortcut
    got = cpu_eval(detmath_cpu, "atan2", y, x)
    ref = np.arctan2(y, x)
    for q, sel in {"I": (y > 0) & (x > 0), "II": (y > 0) & (x < 0), "III": (y < 0) & (x < 0), "IV": (y < 0) & (x > 0)}.items():
        assert sel.sum() > 50000 and ulp_err(got[sel], ref[sel]).max() <= 1.0, q
    # axes and signed zeros: exactly the libm values (pi, pi/2 and their negatives are single roundings of the constants)
    pz, nz, inf = 0.0, -0.0, np.inf
    ys = np.array([pz, nz, pz, nz, pz, nz, pz, nz, 1.0, -1.0, 1.0, -1.0, 3.0, -3.0, 5e-324, -5e-324])
    xs = np.array([pz, pz, nz, nz, 2.0, 2.0, -2.0, -2.0, pz, pz, nz, nz, pz, nz, pz, nz])
    got = cpu_eval(detmath_cpu, "atan2", ys, xs)
    assert np.array_equal(got.view(np.uint64), np.arctan2(ys, xs).view(np.uint64)), (got, np.arctan2(ys, xs))
    # |y / x| beyond 2^64 either way, and the infinities
    ys = np.array([1e300, -1e300, 1e-300, -1e-300, 1e-300, -1e-300, 1e300, -1e300, inf, -inf, inf, -inf, inf, -inf, 1.0, -1.0, 1.0, -1.0])
    xs = np.array([5e-324, -5e-324, 1e300, 1e300, -1e300, -1e300, 1e-300, -1e-300, inf, inf, -inf, -inf, 1.0, 1.0, inf, inf, -inf, -inf])
    got = cpu_eval(detmath_cpu, "atan2", ys, xs)
    ref = np.arctan2(ys, xs)
    assert np.array_equal(np.signbit(got), np.signbit(ref))
    assert (np.abs(got - ref) <= np.spacing(np.abs(ref))).all(), (got, ref)
    assert np.isnan(cpu_eval(detmath_cpu, "atan2", np.array([np.nan, 1.0]), np.array([1.0, np.nan]))).all()


def test_llrint(detmath_cpu):
    """acn_llrint decides the cell of a chess texture: round to nearest, ties to even, for |x| < 2^62 (what the texture code may
    pass: the header)"""
    rng = np.random.default_rng(8)
    k = np.concatenate([np.arange(-9, 10), [2 ** 31, 2 ** 32, 2 ** 51, -2 ** 51, 2 ** 52 - 2, -(2 ** 52) + 2]]).astype(np.float64)
    halves = k + 0.5                                        # both parities, both signs: exact up to 2^52
    x = np.concatenate([halves, np.nextafter(halves, np.inf), np.nextafter(halves, -np.inf), k, [0.0, -0.0, 0.49999999999999994, -0.49999999999999994,
                        5e-324, -5e-324, 2.0 ** 52 + 1, 2.0 ** 53, -(2.0 ** 53), 2.0 ** 62 - 512, -(2.0 ** 62) + 512],
                        rng.uniform(-1e6, 1e6, 200000), rng.normal(size=100000) * np.exp(rng.uniform(-5, 38, 100000))])
    assert np.abs(x).max() < 2.0 ** 62
    got = cpu_eval(detmath_cpu, "llrint", x)
    assert np.array_equal(got, np.rint(x))                  # numpy's rint is nearest-even; integers compare exactly as doubles
    t = cpu_eval(detmath_cpu, "llrint", np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5]))
    assert np.array_equal(t, [0, 2, 2, 4, 0, -2, -2, -4])
