"""The continuous functions of the function-level differential against a float64 restatement of the same formulas - the one leg
that shares no code with the oracle.  Inputs are seeded and kept more than 2^-10 (relative) away from every branch threshold.

The bound is derived, per input, from the function's rounded binary32 operations: the restatement carries every value v with a
bound e on |oracle - v| through the formula (class E below):
  * each binary32 +, -, *, /, sqrt, fma and int->float conversion adds half an ulp, taken as 2^-24 |result| (a normal result);
  * normalize()'s v_rsq_f32 is within 1 ulp of the correctly rounded value (pt_oracle.c): 3 half-ulps; sin / cos carry the
    2 ulps the project documents for its restatement of the platform's (ptmi_detmath.h): 4 half-ulps;
  * the errors of the operands go through each operation's first derivative (exactly for +, - and sqrt; with the operands'
    bounds on both sides for * and /), so cancellation and small denominators widen the bound where they occur;
  * 2 % on top for the second-order terms the first derivative leaves out (inputs whose relative operand error exceeds 2^-6
    anywhere are not used: there "first order" means nothing).
The strict oracle must lie within the bound; the largest |oracle - v| / e seen per function is printed and recorded in
DESIGN.md "Function-level differential"."""
import numpy as np
import pytest

import oracle_ffi as O
import unit_probe_cases as K

f32, u32 = np.float32, np.uint32
H = 2.0 ** -24      # half an ulp, relative
FAR = 2.0 ** -10    # distance kept from every threshold, relative


class E:
    """value and error bound, elementwise over arrays"""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape).copy()
        self.ok = np.ones(self.v.shape, bool)

    def _new(self, v, e, k, *parents):
        r = E(v, e * 1.02 + k * H * np.abs(v))
        for p in parents:
            r.ok = r.ok & p.ok & (p.e <= np.abs(p.v) * 2.0 ** -6 + 1e-300) if isinstance(p, E) else r.ok
        return r

    def __neg__(self):
        r = E(-self.v, self.e)
        r.ok = self.ok
        return r


def _e(x):
    return x if isinstance(x, E) else E(np.float64(f32(x)) if np.isscalar(x) else x)


def add(a, b, k=1):
    a, b = _e(a), _e(b)
    r = E(a.v + b.v, (a.e + b.e) * 1.0 + k * H * np.abs(a.v + b.v))
    r.ok = a.ok & b.ok
    return r


def sub(a, b):
    return add(a, -_e(b))


def mul(a, b, k=1):
    a, b = _e(a), _e(b)
    return a._new(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e, k, a, b)


def div(a, b):
    a, b = _e(a), _e(b)
    q = a.v / b.v
    return a._new(q, (a.e + np.abs(q) * b.e) / np.maximum(np.abs(b.v) - b.e, 1e-300), 1, a, b)


def sqrt(a, k=1):
    a = _e(a)
    lo = np.maximum(a.v - a.e, 0.0)
    r = np.sqrt(np.maximum(a.v, 0.0))
    out = a._new(r, a.e / np.maximum(r + np.sqrt(lo), 1e-300), k, a)
    out.ok &= a.v - a.e > 0
    return out


def fma(a, b, c):
    a, b, c = _e(a), _e(b), _e(c)
    r = E(a.v * b.v + c.v, (np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e) * 1.02 + c.e + H * np.abs(a.v * b.v + c.v))
    r.ok = a.ok & b.ok & c.ok
    return r


def mad(a, b, c):   # strict arithmetic: two roundings
    return add(mul(a, b), c)


def dot(a, b):      # the library's fma chain
    r = mul(a[0], b[0])
    for k in (1, 2, 3):
        r = fma(a[k], b[k], r)
    return r


def rsqrt(a):       # v_rsq_f32: within 1 ulp of the correctly rounded value
    a = _e(a)
    r = 1.0 / np.sqrt(a.v)
    return a._new(r, 0.5 * r / np.maximum(a.v - a.e, 1e-300) * a.e, 3, a)


def normalize(a):
    s = rsqrt(dot(a, a))
    return [mul(x, s) for x in a]


def vec(arr):       # [n,4] binary32 inputs: exact
    return [E(arr[:, k].astype(np.float64)) for k in range(4)]


def maxe(a, floor):  # max(a, floor) is 1-Lipschitz
    a = _e(a)
    r = E(np.maximum(a.v, floor), a.e)
    r.ok = a.ok
    return r


def clamp01(a):
    r = E(np.clip(a.v, 0.0, 1.0), a.e)
    r.ok = a.ok
    return r


RESULTS = {}


def hold(name, got, want, use):
    use = use & want.ok & np.isfinite(want.v) & np.isfinite(want.e)
    assert use.sum() >= 200, (name, int(use.sum()))
    err = np.abs(got.astype(np.float64)[use] - want.v[use])
    bound = want.e[use] + 2.0 ** -149
    ratio = float((err / bound).max())
    RESULTS[name] = (int(use.sum()), ratio, float((want.e[use] / np.maximum(np.abs(want.v[use]), 1e-300)).max() / (2 * H)))
    print(f"{name}: {int(use.sum())} inputs, max |oracle - float64| / bound = {ratio:.3f}, largest bound {RESULTS[name][2]:.1f} ulp")
    assert ratio <= 1.0, f"{name}: the strict oracle leaves its derived bound by a factor {ratio:.3f}"


def fresnel(n1, n2, cos1, inc=None, N=None):
    """fresnel_fraction: (fraction, sin2, refraction direction or None)"""
    sin1 = sqrt(mad(-_e(cos1), cos1, 1.0))
    sin2 = div(mul(n1, sin1), n2)
    cos2 = sqrt(mad(-sin2, sin2, 1.0))
    r_para = div(add(mul(n2, cos1), -mul(n1, cos2)), add(mul(n2, cos1), mul(n1, cos2)))
    r_perp = div(add(mul(n1, cos1), -mul(n2, cos2)), add(mul(n1, cos1), mul(n2, cos2)))
    frac = mul(add(mul(r_para, r_para), mul(r_perp, r_perp)), 0.5, k=0)
    refr = None
    if inc is not None:
        ratio = div(n1, n2)
        side = add(mul(ratio, cos1), -cos2)
        refr = [add(mul(inc[k], ratio), mul(N[k], side)) for k in range(4)]
    return frac, sin2, refr


def unit_vectors(rs, n):
    v = rs.normal(size=(n, 4))
    v[:, 3] = 0
    v /= np.linalg.norm(v, axis=1)[:, None]
    return v.astype(f32)


@pytest.fixture(scope="module")
def lib(built):
    return O.oracle(False)


def test_fresnel_and_brdf(lib):
    rs = np.random.RandomState(20)
    n = 1500
    N = unit_vectors(rs, n)
    inc = -(N + 0.9 * unit_vectors(rs, n)).astype(f32)
    inc = (inc / np.linalg.norm(inc, axis=1)[:, None]).astype(f32)
    refl = unit_vectors(rs, n)
    rows = [[inc[i], N[i], refl[i], K.U((1, 3)[i % 2]), K.U((i // 2) % 2)] for i in range(n)]
    cases = K._rows(rows, K.MATERIAL_WORDS)
    out = K.oracle_material(lib, cases).view(f32)
    cos1 = -dot(vec(inc), vec(N))
    away_from_one = lambda s: np.abs(s.v - 1.0) > FAR + s.e
    g, s2, _ = fresnel(1.0, f32(1.55), cos1)
    hold("fresnel glass", out[:, 0], g, away_from_one(s2) & (s2.v < 1) & (cos1.v > FAR))
    cv = clamp01(cos1)
    v, s2, _ = fresnel(1.0, f32(3.0), cv)
    inside = (cos1.v > FAR) & (cos1.v < 1 - FAR)
    hold("fresnel varnish", out[:, 1], v, inside & (s2.v < 1))
    in_water = cases[:, 13] == 1
    for flag, n1, n2, name in ((0, 1.0, f32(1.333), "fresnel water (from air)"), (1, f32(1.333), 1.0, "fresnel water (from inside)")):
        w, s2, refr = fresnel(n1, n2, cos1, vec(inc), vec(N))
        use = (in_water == bool(flag)) & away_from_one(s2) & (s2.v < 1) & (cos1.v > FAR)
        hold(name, out[:, 2], w, use)
        for k in range(3):
            hold(name + f" refraction[{k}]", out[:, 3 + k], refr[k], use)
    water = cases[:, 12] == 1
    denom = add(mul(f32(0.8), dot(vec(inc), vec(refl))), 1.0)
    num = add(1.0, -mul(f32(0.8), f32(0.8)))
    brdf = div(num, mul(mul(mul(4.0, f32(3.14159265)), denom), denom))
    hold("brdf water", out[:, 8], brdf, water)
    hold("brdf varnish", out[:, 8], mul(add(1.0, -v), f32(0.31830988618)), ~water & inside & (s2.v < 10))


def test_light_power(lib):
    rs = np.random.RandomState(21)
    n = 6000
    pos = np.concatenate([rs.uniform(-4, 4, (n, 3)), np.ones((n, 1))], axis=1).astype(f32)
    p = np.concatenate([rs.uniform(-4, 4, (n, 3)), np.ones((n, 1))], axis=1).astype(f32)
    direction, N = unit_vectors(rs, n), unit_vectors(rs, n)
    toward_p = (p - pos) / np.linalg.norm(p - pos, axis=1)[:, None]
    direction = (toward_p + np.where(np.arange(n) % 2, 0.25, 1.0)[:, None] * direction).astype(f32)   # lights that see p, in and between the cones
    power = rs.uniform(0.5, 50, n).astype(f32)
    ci, co = rs.uniform(0.85, 0.97, n).astype(f32), rs.uniform(0.1, 0.5, n).astype(f32)
    kind = np.arange(n) % 3
    rows = [[pos[i], direction[i], power[i], ci[i], co[i], K.U(kind[i]), p[i], N[i]] for i in range(n)]
    cases = K._rows(rows, K.LIGHT_WORDS)
    out = K.oracle_light(lib, cases).view(f32)[:, 0]
    P, POS, D, NN = vec(p), vec(pos), vec(direction), vec(N)
    hold("light directional", out, mul(power, maxe(dot([-x for x in D], NN), 0.0)), kind == 0)
    d = [sub(P[k], POS[k]) for k in range(4)]
    toward = normalize([sub(POS[k], P[k]) for k in range(4)])
    hold("light point", out, mul(div(power, dot(d, d)), maxe(dot(toward, NN), 0.0)), kind == 1)
    lrd = normalize(d)
    cos_angle = dot(lrd, D)
    facing = maxe(-dot(lrd, NN), 0.0)
    spot = kind == 2
    far = lambda t: np.abs(cos_angle.v - t) > FAR * np.abs(t) + cos_angle.e
    hold("light spot, inner cone", out, mul(power, facing), spot & (cos_angle.v > ci) & far(ci))
    between = div(mul(power, sub(cos_angle, co)), sub(ci, co))
    hold("light spot, between the cones", out, mul(between, facing), spot & (cos_angle.v < ci) & (cos_angle.v > co) & far(ci) & far(co))


def test_hemisphere_direction(lib):
    rs = np.random.RandomState(22)
    n = 3000
    seeds = rs.randint(1, 2 ** 31 - 1, n).astype(np.int64)
    N = unit_vectors(rs, n)
    N[::5] = np.array([0, 0, 1, 0], f32)
    N[1::5] = np.array([0, 0, -1, 0], f32)
    rows = [[K.U(int(seeds[i])), N[i]] + [K.U(0)] * 5 for i in range(n)]
    cases = K._rows(rows, K.SAMPLING_WORDS)
    out = K.oracle_sampling(lib, cases)[:, 4:8].view(f32)
    s1 = (K.LCG_A * seeds) & K.LCG_MASK
    s2 = (K.LCG_A * s1) & K.LCG_MASK
    u1, u2 = mul(E(s1.astype(np.float64)), 1.0, k=1), mul(E(s2.astype(np.float64)), 1.0, k=1)   # int -> float rounds; / 2^31 is exact
    sx, sy = add(mul(u1, 2.0 ** -30, k=0), -1.0), add(mul(u2, 2.0 ** -30, k=0), -1.0)
    x, y = sx.v, sy.v
    far = lambda a, b: np.abs(a - b) > FAR * np.maximum(np.abs(a), np.abs(b)) + 4 * H
    use = far(x, -y) & far(x, y) & (np.abs(x) > 1e-4 * (1 + FAR)) & (np.abs(y) > 1e-4 * (1 + FAR)) & far(y, 0 * y)
    upper = x > -y
    a, b, c, d = upper & (x > y), upper & ~(x > y), ~upper & (x < y), ~upper & ~(x < y)

    def pick(mask_values):
        v, e = np.zeros(n), np.zeros(n)
        for m, val in mask_values:
            v[m], e[m] = val.v[m], val.e[m]
        return E(v, e)
    q_yx, q_xy = div(sy, sx), div(sx, sy)
    theta = pick([(a & (y > 0), q_yx), (a & ~(y > 0), add(8.0, q_yx)), (b, sub(2.0, q_xy)), (c, add(4.0, q_yx)), (d, sub(6.0, q_yx))])
    r = pick([(a, sx), (b, sy), (c, -sx), (d, -sy)])
    theta = mul(theta, np.float64(f32(3.14159265)) / 4)
    r = mul(r, 0.999)                                   # one rounding: the double product converted
    cs = E(np.cos(theta.v), theta.e + 4 * H * np.abs(np.cos(theta.v)))
    sn = E(np.sin(theta.v), theta.e + 4 * H * np.abs(np.sin(theta.v)))
    dx, dy = mul(r, cs), mul(r, sn)
    z = sqrt(add(mul(-dy, dy), add(mul(-dx, dx), 1.0)))
    v = [dx, dy, z, E(np.zeros(n))]
    nz = N[:, 2].astype(np.float64)
    use &= np.abs(np.abs(nz) - 0.9999) > FAR
    up_, down_ = nz > 0.9999, nz < -0.9999
    NN = vec(N)
    zero = E(np.zeros(n))
    sn4 = normalize([-NN[1], NN[0], zero, zero])
    cr = [fma(NN[1], sn4[2], mul(sn4[1], -NN[2])), fma(NN[2], sn4[0], mul(sn4[2], -NN[0])), fma(NN[0], sn4[1], mul(sn4[0], -NN[1])), zero]
    tn4 = normalize(cr)
    world = normalize([dot([sn4[k], tn4[k], NN[k], zero], v) for k in range(3)] + [zero])
    for k in range(3):
        want = pick([(up_, v[k]), (down_, -v[k]), (~up_ & ~down_, world[k])])
        want.ok = v[k].ok & world[k].ok | ((up_ | down_) & v[k].ok)
        hold(f"hemisphere direction[{k}]", out[:, k], want, use)
