"""SO(3) for the yardsticks of the relative-pose factors and the joint pose priors: Exp, Log and the inverse right and left
Jacobians, evaluated with mpmath at 60 digits and returned as float64.

Nothing here shares a formula with the kernels (rp_log, rp_jrinv, jp_jlinv in surikatoko_amd/csrc/srk_ba_kernels.hip):

    exp(phi)      Rodrigues; the identity, exactly, at phi = 0
    log(M)        through the unit quaternion of M, the largest of its four components taken first, so it is valid on [0, pi];
                  a matrix whose antisymmetric part is exactly zero and whose trace is nearest 3 gives exactly [0, 0, 0]
    jr_inv(phi)   central difference of d -> log(exp(phi) exp(d)) with step 1e-20: no closed form
    jl_inv(phi)   central difference of d -> log(exp(d) exp(phi))

With 60 digits and a step of 1e-20 the differences are off by about 1e-40 (truncation h^2, rounding 1e-60 / h), so what they
return is the correctly rounded Jacobian for every angle below pi - 1e-19.  At pi itself Log is not differentiable and the
Jacobians are not defined; log() there returns pi times the axis with the sign the quaternion's rounding gives.

The numpy restatement of the kernels' formulas lives here as well (kernel_log, kernel_jr_inv, kernel_jl_inv), for
tests/test_so3_cpu.py to hold against the functions above, and is used for nothing else.  kernel_log_old and kernel_k_old are
the formulas before the path near pi and the half-angle form were added: that test shows that they miss its bounds.

Results are cached by the bytes of the argument: the LM yardsticks ask for the same residuals again and again."""
import functools

import mpmath as mp
import numpy as np

DPS = 60
STEP = "1e-20"


def _skew(p):
    return mp.matrix([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])


def _exp(p):
    """Rodrigues on three mpf"""
    t2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2]
    if t2 == 0:
        return mp.eye(3)
    t = mp.sqrt(t2)
    P = _skew(p)
    return mp.eye(3) + (mp.sin(t) / t) * P + ((1 - mp.cos(t)) / t2) * (P * P)


def _log(M):
    """rotation vector of the 3 x 3 mp matrix M through its unit quaternion (w, x, y, z), the largest component first"""
    d = [M[0, 0], M[1, 1], M[2, 2]]
    four = [1 + d[0] + d[1] + d[2], 1 + d[0] - d[1] - d[2], 1 - d[0] + d[1] - d[2], 1 - d[0] - d[1] + d[2]]  # 4 w^2, 4 x^2, ...
    k = max(range(4), key=lambda i: four[i])
    s = 2 * mp.sqrt(four[k])  # 4 |q_k|
    if k == 0:
        q = [s / 4, (M[2, 1] - M[1, 2]) / s, (M[0, 2] - M[2, 0]) / s, (M[1, 0] - M[0, 1]) / s]
    elif k == 1:
        q = [(M[2, 1] - M[1, 2]) / s, s / 4, (M[0, 1] + M[1, 0]) / s, (M[0, 2] + M[2, 0]) / s]
    elif k == 2:
        q = [(M[0, 2] - M[2, 0]) / s, (M[0, 1] + M[1, 0]) / s, s / 4, (M[1, 2] + M[2, 1]) / s]
    else:
        q = [(M[1, 0] - M[0, 1]) / s, (M[0, 2] + M[2, 0]) / s, (M[1, 2] + M[2, 1]) / s, s / 4]
    if q[0] < 0:
        q = [-x for x in q]
    n = mp.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    if n == 0:
        return [mp.mpf(0)] * 3
    f = 2 * mp.atan2(n, q[0]) / n
    return [f * q[1], f * q[2], f * q[3]]


def _mat(M):
    return mp.matrix([[mp.mpf(float(M[r, c])) for c in range(3)] for r in range(3)])


def _vec(p):
    return [mp.mpf(float(x)) for x in p]


@functools.lru_cache(maxsize=None)
def _exp_bytes(b):
    with mp.workdps(DPS):
        E = _exp(_vec(np.frombuffer(b, dtype=np.float64)))
        return np.array([[float(E[r, c]) for c in range(3)] for r in range(3)])


@functools.lru_cache(maxsize=None)
def _log_bytes(b):
    with mp.workdps(DPS):
        return np.array([float(x) for x in _log(_mat(np.frombuffer(b, dtype=np.float64).reshape(3, 3)))])


@functools.lru_cache(maxsize=None)
def _jinv_bytes(b, left):
    with mp.workdps(DPS):
        E = _exp(_vec(np.frombuffer(b, dtype=np.float64)))
        h = mp.mpf(STEP)
        J = np.zeros((3, 3))
        for c in range(3):
            d = [mp.mpf(0)] * 3
            d[c] = h
            Dp, Dm = _exp(d), _exp([-x for x in d])
            lp = _log(Dp * E if left else E * Dp)
            lm = _log(Dm * E if left else E * Dm)
            for r in range(3):
                J[r, c] = float((lp[r] - lm[r]) / (2 * h))
        return J


def _key(a, n):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64)).reshape(n) + 0.0  # -0.0 -> 0.0: one key for both
    return a.tobytes()


def exp(phi):
    """[3][3]: the rotation of the rotation vector phi"""
    return _exp_bytes(_key(phi, 3)).copy()


def log(M):
    """[3]: the rotation vector of the rotation matrix M, angle in [0, pi]"""
    return _log_bytes(_key(M, 9)).copy()


def jr_inv(phi):
    """inverse right Jacobian of SO(3): Log(Exp(phi) Exp(d)) = phi + Jr^-1(phi) d + O(d^2)"""
    return _jinv_bytes(_key(phi, 3), False).copy()


def jl_inv(phi):
    """inverse left Jacobian of SO(3): Log(Exp(d) Exp(phi)) = phi + Jl^-1(phi) d + O(d^2)"""
    return _jinv_bytes(_key(phi, 3), True).copy()


# ------------------------------------------------------------------ the kernels' formulas in numpy, for tests/test_so3_cpu.py alone

LOG_PI_COS = -0.9   # rp_log / so3_log: the axis comes from the symmetric part where the cosine is below this
K_HALF_T2 = 2.25    # rp_jrinv / jp_jlinv: the half-angle form of k where the squared angle is at least this

# The residual angles every sweep runs, on the CPU and on the GPU: zero, both sides of every switch of the three formulas (the
# series of Log below sin = 1e-4, the series of k below 1e-3 rad, the half-angle form of k from 1.5 rad, the symmetric-part
# axis from acos(-0.9) = 2.6906 rad), the range between them, and the approach to pi.  pi itself has tests of its own.
SWEEP = [0.0, 1e-12, 1e-8, 0.99e-4, 1.01e-4, 0.99e-3, 1.01e-3, 0.05, 1.0, 1.49, 1.51, np.pi / 2, 2.0, 2.6, 2.68, 2.70, 2.8, 3.0,
         np.pi - 1e-3, np.pi - 1e-6, np.pi - 1e-9]
# one angle below and one above each switch
AT_SWITCHES = [0.99e-4, 1.01e-4, 0.99e-3, 1.01e-3, 1.49, 1.51, 2.68, 2.70]


def axes(n, seed=5):
    """n unit vectors: a coordinate axis (exact zeros in the antisymmetric part) and n - 1 seeded ones"""
    a = np.random.RandomState(seed).normal(size=(n - 1, 3))
    return np.concatenate([[[0.0, 1.0, 0.0]], a / np.linalg.norm(a, axis=1)[:, None]])


def kernel_log_old(M):
    """rp_log before the path near pi: the antisymmetric part alone"""
    v = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    s2 = float(v @ v)
    sn = float(np.sqrt(s2))
    cs = 0.5 * (M[0, 0] + M[1, 1] + M[2, 2] - 1.0)
    if sn < 1e-4 and cs > 0:
        return v * (1.0 + s2 / 6.0 + 3.0 * s2 * s2 / 40.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return v * (np.arctan2(sn, cs) / sn)


def kernel_log(M):
    """rp_log and so3_log, line for line"""
    M = np.asarray(M, dtype=np.float64)
    v = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    s2 = float(v @ v)
    sn = float(np.sqrt(s2))
    cs = 0.5 * (M[0, 0] + M[1, 1] + M[2, 2] - 1.0)
    if cs < LOG_PI_COS:
        if M[0, 0] >= M[1, 1] and M[0, 0] >= M[2, 2]:
            a = np.array([M[0, 0] - cs, 0.5 * (M[1, 0] + M[0, 1]), 0.5 * (M[2, 0] + M[0, 2])])
        elif M[1, 1] >= M[2, 2]:
            a = np.array([0.5 * (M[0, 1] + M[1, 0]), M[1, 1] - cs, 0.5 * (M[2, 1] + M[1, 2])])
        else:
            a = np.array([0.5 * (M[0, 2] + M[2, 0]), 0.5 * (M[1, 2] + M[2, 1]), M[2, 2] - cs])
        t = np.arctan2(sn, cs)
        f = (-t if float(a @ v) < 0 else t) / np.sqrt(float(a @ a))
        return f * a
    if sn < 1e-4 and cs > 0:
        return v * (1.0 + s2 / 6.0 + 3.0 * s2 * s2 / 40.0)
    return v * (np.arctan2(sn, cs) / sn)


def kernel_k_old(t2):
    if t2 < 1e-6:
        return 1.0 / 12.0 + t2 / 720.0
    t = np.sqrt(t2)
    return 1.0 / t2 - (1.0 + np.cos(t)) / (2.0 * t * np.sin(t))


def kernel_k(t2):
    """the coefficient of [phi]x^2 in rp_jrinv and jp_jlinv"""
    if t2 < 1e-6:
        return 1.0 / 12.0 + t2 / 720.0
    t = np.sqrt(t2)
    if t2 >= K_HALF_T2:
        return 1.0 / t2 - 1.0 / (2.0 * t * np.tan(0.5 * t))
    return 1.0 / t2 - (1.0 + np.cos(t)) / (2.0 * t * np.sin(t))


def _kernel_jinv(p, sg, k_of):
    p = np.asarray(p, dtype=np.float64)
    t2 = float(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
    k = k_of(t2)
    h = 0.5 * sg
    return np.array([[1.0 + k * (p[0] * p[0] - t2), -h * p[2] + k * p[0] * p[1], h * p[1] + k * p[0] * p[2]],
                     [h * p[2] + k * p[0] * p[1], 1.0 + k * (p[1] * p[1] - t2), -h * p[0] + k * p[1] * p[2]],
                     [-h * p[1] + k * p[0] * p[2], h * p[0] + k * p[1] * p[2], 1.0 + k * (p[2] * p[2] - t2)]])


def kernel_jr_inv(phi, k_of=kernel_k):
    """rp_jrinv: I + [phi]x / 2 + k [phi]x^2, [phi]x^2 = phi phi^T - t2 I"""
    return _kernel_jinv(phi, 1.0, k_of)


def kernel_jl_inv(phi, k_of=kernel_k):
    """jp_jlinv: I - [phi]x / 2 + k [phi]x^2"""
    return _kernel_jinv(phi, -1.0, k_of)
