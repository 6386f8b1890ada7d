"""Long-double references, the ulp measure and the input sets of the device-math tests (tests/test_gpu_device_math.py
runs the kernels' own functions on these inputs; tests/test_device_math_cpu.py checks this file against 200-bit mpmath).

np.longdouble is the x87 80-bit format here (64-bit mantissa): 2^-11 of a double's ulp, enough to resolve the 1.5 - 2 ulp
gates of the hand-written float64 routines of csrc/philox.hpp and csrc/jump_math.hpp."""
import numpy as np

LD = np.longdouble
TWO53 = 9007199254740992.0
# pi to 64 bits: the sum of its two leading float64 pieces, rounded once (both pieces are exact in long double)
PI_LD = LD(3.141592653589793) + LD(1.2246467991473532e-16)
SQRT_HALF = float(np.array([0x3fe6a09e667f3bcd], dtype=np.uint64).view(np.float64)[0])   # neg_log_unit's `low` switch
LN_DBL_MAX = 709.782712893384          # exp overflows above it
LN_DBL_MIN = -708.3964185322641        # exp is subnormal below it
_MIN64 = np.int64(-2 ** 63)


# ---------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------
def neg_log_ref(u):
    """-log(u) in long double"""
    return -np.log(np.asarray(u, dtype=np.float64).astype(LD))


def exp_ref(h):
    """exp(h) in long double (its exponent range holds every finite double's exponential that is not 0 or inf in double)"""
    with np.errstate(over='ignore', under='ignore'):
        return np.exp(np.asarray(h, dtype=np.float64).astype(LD))


def to_f64(x):
    """long double -> float64, round to nearest: into the subnormal range, to 0 and to inf"""
    with np.errstate(over='ignore', under='ignore'):
        return np.asarray(x, dtype=LD).astype(np.float64)


def sincospi_ref(t):
    """(sin(pi t), cos(pi t)) in long double for t in [0, 2]: the reduction n = rint(2 t), r = t - n / 2 is exact in
    float64 (|r| <= 1/4), sin and cos of pi r are taken in long double, and the quadrant is turned on the host."""
    t = np.asarray(t, dtype=np.float64)
    n = np.rint(2.0 * t)
    r = t - 0.5 * n
    x = PI_LD * r.astype(LD)
    s0, c0 = np.sin(x), np.cos(x)
    q = n.astype(np.int64) & 3
    s = np.where(q == 0, s0, np.where(q == 1, c0, np.where(q == 2, -s0, -c0)))
    c = np.where(q == 0, c0, np.where(q == 1, -s0, np.where(q == 2, -c0, s0)))
    return s, c


def box_muller_ref(u1, u2):
    """(r cos(2 pi u2), r sin(2 pi u2), r) in long double, r = sqrt(-2 log u1)"""
    r = np.sqrt(LD(2) * neg_log_ref(u1))
    s, c = sincospi_ref(2.0 * np.asarray(u2, dtype=np.float64))
    return r * c, r * s, r


# ---------------------------------------------------------------------------------------------
# the measure
# ---------------------------------------------------------------------------------------------
def ulp_err(got, want_ld):
    """|got - want| in ulps of the float64 the reference rounds to: spacing(float64(want)), which is 2^-1074 in the
    subnormal range and at 0.  A reference that rounds to inf (or is NaN) asks for exactly that: 0 or inf."""
    got = np.asarray(got, dtype=np.float64)
    want_ld = np.asarray(want_ld, dtype=LD)
    w64 = to_f64(want_ld)
    err = np.full(got.shape, np.inf)
    both_nan = np.isnan(got) & np.isnan(w64)
    same_inf = np.isinf(w64) & (got == w64)
    fin = np.isfinite(got) & np.isfinite(w64)
    err[both_nan | same_inf] = 0.0
    with np.errstate(invalid='ignore', over='ignore'):
        d = np.abs(got.astype(LD) - want_ld) / np.spacing(np.abs(w64)).astype(LD)
    err[fin] = d[fin].astype(np.float64)
    return err


# ---------------------------------------------------------------------------------------------
# input sets
# ---------------------------------------------------------------------------------------------
def neighbours(x, k=64):
    """x and the k float64 values on either side of it (across 0 and the binade ends), ascending"""
    i = np.array([x], dtype=np.float64).view(np.int64)[0]
    o = (_MIN64 - i) if i < 0 else i                      # monotone integer image of the doubles (-0.0 and +0.0 -> 0)
    o = o + np.arange(-k, k + 1, dtype=np.int64)
    bits = np.where(o < 0, _MIN64 - o, o)
    return bits.view(np.float64)


def on_grid(u):
    """the multiples of 2^-53 in (0, 1] among u: what u53() can return"""
    u = np.asarray(u, dtype=np.float64)
    j = u * TWO53
    return u[(u > 0) & (u <= 1) & (j == np.rint(j))]


def log_edges():
    """the edge subset of the log inputs: both ends of (0, 1], every binade end and every `low` switch"""
    parts = [np.arange(1, 65) / TWO53, 1.0 - np.arange(0, 65) / TWO53]
    for e in range(1, 54):
        for x in (2.0 ** -e, 2.0 ** -(e - 1), SQRT_HALF * 2.0 ** -(e - 1)):
            parts.append(on_grid(neighbours(x)))
        # in the small binades the grid is coarser than 64 doubles: the grid points around the binade end and the switch
        j0 = np.floor(SQRT_HALF * 2.0 ** -(e - 1) * TWO53)
        parts.append(on_grid((j0 + np.arange(-1, 3)) / TWO53))
        parts.append(on_grid((2.0 ** (53 - e) + np.arange(-2, 3)) / TWO53))
    return np.unique(np.concatenate(parts))


def log_inputs():
    rs = np.random.RandomState(20240531)
    j = np.maximum(1.0, np.rint(np.exp(rs.uniform(np.log(1.0 / TWO53), 0.0, 1 << 16)) * TWO53))
    return np.unique(np.concatenate([np.arange(1, 4097) / TWO53, 1.0 - np.arange(0, 4097) / TWO53, log_edges(), j / TWO53]))


def _in_angle_range(t):
    return t[(t >= 0) & (t <= 2)]


def angle_edges():
    """the n switches and octants k/8, and the cosine's qx split |pi r| = 0.3, with 64 neighbours on either side"""
    parts = [_in_angle_range(neighbours(k / 8.0)) for k in range(17)]
    for n in range(5):
        for sgn in (-1.0, 1.0):
            parts.append(_in_angle_range(neighbours(0.5 * n + sgn * 0.3 / np.pi)))
    return np.unique(np.concatenate(parts))


def angle_inputs():
    rs = np.random.RandomState(20240601)
    return np.unique(np.concatenate([angle_edges(), 2.0 * log_inputs(), rs.uniform(0.0, 2.0, 1 << 16)]))


EXP_EDGES = (-745.1332, -708.3964, -708.0, -0.5 * np.log(2.0), 0.0, 708.0, 709.0, 709.7827, -1100.0, 1100.0)
EXP_SPECIALS = (0.0, -0.0, 1e-300, -1e-300, 1e308, -1e308, np.inf, -np.inf, np.nan)


def exp_edges():
    return np.concatenate([neighbours(x) for x in EXP_EDGES] + [np.array(EXP_SPECIALS)])


def exp_inputs():
    return np.concatenate([np.arange(-760.0, 720.0, 0.0137), exp_edges()])


BM_U1_CENTRES = (2.0 ** -53, 2.0 ** -52, 2.0 ** -40, 2.0 ** -20, 0.5, 1.0 - 2.0 ** -53, 1.0)


def box_muller_inputs():
    """(u1, u2): the tails and the middle of the radius crossed with every angle edge, plus 2^16 pairs of u53() values"""
    u1e = np.unique(np.concatenate([on_grid(neighbours(x, 8)) for x in BM_U1_CENTRES]))
    t = angle_edges()
    u2e = 0.5 * t[t > 0]
    u2e = u2e[(u2e > 0) & (2.0 * u2e == t[t > 0])]        # (an odd subnormal has no half)
    rs = np.random.RandomState(20240602)
    ur = (rs.randint(0, 1 << 53, size=(2, 1 << 16), dtype=np.int64).astype(np.float64) + 1.0) / TWO53
    u1 = np.concatenate([np.repeat(u1e, u2e.size), ur[0]])
    u2 = np.concatenate([np.tile(u2e, u1e.size), ur[1]])
    return u1, u2
