"""Sequential restatement of optimize::graph_optimizer::optimize as DESIGN.md 3.19 fixes it (rules G1 to G11): one edge after the other, one
trial after the other. Pure Python on purpose: a Python float is an IEEE f64 and every operation below rounds once, so the results are the
bits the rules ask for. No numpy in the arithmetic; imports nothing of the product. Rule 2's exponential and its sin / cos / exp are
tests/transform_ref.py's; det_log (G4) and det_acos (include/ovs_detmath.h) are restated here.

A scene is a dict: V, nc (lists of (R 9 row-major, t 3, s)), fixed (list of 0 / 1), edges (list of (i, j)), meas (list of (R, t, s)),
fix_scale, num_iter, pcg_max_iter, lm_ref (list of vertex or -1), lm_pos (list of 3-lists)."""
import math
import struct
from fractions import Fraction

from sim3_ref import _div, _sqrt, bits, dot3  # noqa: F401
from transform_ref import _sincos, exp_apply, with_inverse

EPS, DELTA, TOL, LAMBDA0, DBL_MAX = 1e-5, 1e-9, 1e-6, 1e-16, 1.7976931348623157e308
NAN, INF = float("nan"), float("inf")

# ---- G4
LN2_HI, LN2_LO = float.fromhex("0x1.62e42fee00000p-1"), float.fromhex("0x1.a39ef35793c76p-33")   # ln 2 cut to 32 significant bits, and the rest
SQRT2 = float.fromhex("0x1.6a09e667f3bcdp+0")
L_K = [float(Fraction(2, 2 * j + 1)) for j in range(11)]   # L_K[1 .. 10] are used


def _from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def det_log(x):
    if not x > 0.0 or not x < INF:
        return NAN
    k = 0
    if x < 2.0 ** -1022:
        x = x * 2.0 ** 54
        k = -54
    u = bits(x)
    k += (u >> 52) - 1023
    m = _from_bits((u & 0x000fffffffffffff) | 0x3ff0000000000000)
    if m > SQRT2:
        m = m * 0.5
        k += 1
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    p = L_K[10]
    for j in range(9, 0, -1):
        p = L_K[j] + z * p
    R = z * p
    h = 0.5 * (f * f)
    dk = float(k)
    return dk * LN2_HI - ((h - (s * (h + R) + dk * LN2_LO)) - f)


# ---- ovs_det_acos (fdlibm's e_acos.c as the header restates it)
_PS = [1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01, -4.00555345006794114027e-02,
       7.91534994289814532176e-04, 3.47933107596021167570e-05]
_QS = [-2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02]
_PI, _PIO2_HI, _PIO2_LO = 3.14159265358979311600e+00, 1.57079632679489655800e+00, 6.12323399573676603587e-17


def _asin_pq(t):
    p = t * (_PS[0] + t * (_PS[1] + t * (_PS[2] + t * (_PS[3] + t * (_PS[4] + t * _PS[5])))))
    q = 1.0 + t * (_QS[0] + t * (_QS[1] + t * (_QS[2] + t * _QS[3])))
    return p / q


def det_acos(x):
    if x != x:
        return x + x
    ax, neg = abs(x), math.copysign(1.0, x) < 0
    if ax >= 1.0:
        if ax == 1.0:
            return _PI + 2.0 * _PIO2_LO if neg else 0.0
        return NAN
    if ax < 0.5:
        if ax < 6.938893903907228e-18:
            return _PIO2_HI + _PIO2_LO
        z = x * x
        r = _asin_pq(z)
        return _PIO2_HI - (x - (_PIO2_LO - x * r))
    if neg:
        z = (1.0 + x) * 0.5
        r = _asin_pq(z)
        s = math.sqrt(z)
        w = r * s - _PIO2_LO
        return _PI - 2.0 * (s + w)
    z = (1.0 - x) * 0.5
    s = math.sqrt(z)
    df = _from_bits(bits(s) & 0xffffffff00000000)
    c = (z - df * df) / (s + df)
    r = _asin_pq(z)
    w = r * s + c
    return 2.0 * (df + w)


# ---- G1: states are transform_ref's dicts (R, t, s, s21, t21)
def state(R, t, s):
    return with_inverse(R, t, s)


def compose(A, B):
    R = [(A["R"][3 * i] * B["R"][j] + A["R"][3 * i + 1] * B["R"][3 + j]) + A["R"][3 * i + 2] * B["R"][6 + j] for i in range(3) for j in range(3)]
    t = [A["s"] * dot3(A["R"][3 * i], A["R"][3 * i + 1], A["R"][3 * i + 2], *B["t"]) + A["t"][i] for i in range(3)]
    return dict(R=R, t=t, s=A["s"] * B["s"])


def compose_inverse(A, B):
    R = [(A["R"][3 * i] * B["R"][3 * j] + A["R"][3 * i + 1] * B["R"][3 * j + 1]) + A["R"][3 * i + 2] * B["R"][3 * j + 2]
         for i in range(3) for j in range(3)]
    t = [A["s"] * dot3(A["R"][3 * i], A["R"][3 * i + 1], A["R"][3 * i + 2], *B["t21"]) + A["t"][i] for i in range(3)]
    return dict(R=R, t=t, s=A["s"] * B["s21"])


# ---- G3
def log_parts(T):
    """(e, branch): the seven of log(T) and which of the four branches the coefficients took."""
    R, s = T["R"], T["s"]
    sigma = det_log(s)
    d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0)
    r0, r1, r2 = R[7] - R[5], R[2] - R[6], R[3] - R[1]
    small_t, small_s = d > 1.0 - EPS, abs(sigma) < EPS
    theta, kf = 0.0, 0.5
    if not small_t:
        theta = det_acos(d)
        kf = _div(theta, 2.0 * _sqrt(1.0 - d * d))
    w0, w1, w2 = kf * r0, kf * r1, kf * r2
    Om = [0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0]
    Om2 = [(Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j]) + Om[3 * i + 2] * Om[6 + j] for i in range(3) for j in range(3)]
    sn, cs = _sincos(theta)
    th2 = theta * theta
    if small_s:
        C = 1.0
        if small_t:
            A, B = 0.5, 1.0 / 6.0
        else:
            A, B = _div(1.0 - cs, th2), _div(theta - sn, th2 * theta)
    else:
        C = _div(s - 1.0, sigma)
        sg2 = sigma * sigma
        if small_t:
            A = _div((sigma - 1.0) * s + 1.0, sg2)
            B = _div((0.5 * sg2 - sigma + 1.0) * s - 1.0, sg2 * sigma)
        else:
            a, b, c = s * sn, s * cs, th2 + sg2
            A = _div(a * sigma + (1.0 - b) * theta, theta * c)
            B = _div(C - _div((b - 1.0) * sigma + a * theta, c), th2)
    W = [(A * Om[k] + B * Om2[k]) + C * (1.0 if k % 4 == 0 else 0.0) for k in range(9)]
    c00, c01, c02 = W[4] * W[8] - W[5] * W[7], W[5] * W[6] - W[3] * W[8], W[3] * W[7] - W[4] * W[6]
    c10, c11, c12 = W[2] * W[7] - W[1] * W[8], W[0] * W[8] - W[2] * W[6], W[1] * W[6] - W[0] * W[7]
    c20, c21, c22 = W[1] * W[5] - W[2] * W[4], W[2] * W[3] - W[0] * W[5], W[0] * W[4] - W[1] * W[3]
    det = dot3(W[0], W[1], W[2], c00, c01, c02)
    t = T["t"]
    e = [w0, w1, w2, _div(dot3(c00, c10, c20, *t), det), _div(dot3(c01, c11, c21, *t), det), _div(dot3(c02, c12, c22, *t), det), sigma]
    return e, ("small" if small_t else "large") + "_theta_" + ("small" if small_s else "large") + "_sigma"


LOG_PATHS = set()   # the branches every evaluation of this process has taken (the scene set's coverage test reads it)


def log_of(T):
    e, branch = log_parts(T)
    LOG_PATHS.add(branch)
    return e


def edge_error(M, Si, Sj):
    return log_of(compose_inverse(compose(M, Si), Sj))


def chi_of(e):
    s = e[0] * e[0]
    for k in range(1, 7):
        s = s + e[k] * e[k]
    return s


def tree(values):
    """Rule 6 over a list of (index, value): partial j of 64 takes the indices j, j + 64, ... from 0.0; then part[j] += part[j + d]."""
    part = [0.0] * 64
    for i, v in values:
        part[i % 64] = part[i % 64] + v
    d = 32
    while d:
        for j in range(d):
            part[j] = part[j] + part[j + d]
        d >>= 1
    return part[0]


def dot7(a, b):
    s = a[0] * b[0]
    for k in range(1, 7):
        s = s + a[k] * b[k]
    return s


def unit(d, step):
    return [step if k == d else 0.0 for k in range(7)]


class Optimizer:
    """One run of G5 to G9 and G11, with what the tests ask about it: the blocks of the first linearisation, the trial log, the paths."""

    def __init__(self, scene):
        self.q = scene
        self.n_v, self.n_e = len(scene["V"]), len(scene["edges"])
        self.fixed = list(scene["fixed"])
        self.free = [v for v in range(self.n_v) if not self.fixed[v]]
        self.fix_scale = bool(scene["fix_scale"])
        self.inc = [[] for _ in range(self.n_v)]           # G7's incidence lists: (edge, side), ascending edge index
        for ei, (i, j) in enumerate(scene["edges"]):
            self.inc[i].append((ei, 0))
            self.inc[j].append((ei, 1))
        self.M = [dict(R=list(R), t=list(t), s=s) for R, t, s in scene["meas"]]
        self.paths, self.trial_log, self.first = set(), [], None

    def linearize(self, V):
        q, k = self.q, 1.0 / (2.0 * DELTA)
        E, J, chi_e = [], [], []
        for ei, (i, j) in enumerate(q["edges"]):
            M, Si, Sj = self.M[ei], V[i], V[j]
            e = edge_error(M, Si, Sj)
            Ji = Jj = None
            if not self.fixed[i]:
                Ji = [[0.0] * 7 for _ in range(7)]
                for d in range(7):
                    ep = edge_error(M, exp_apply(unit(d, DELTA), self.fix_scale, Si), Sj)
                    em = edge_error(M, exp_apply(unit(d, -DELTA), self.fix_scale, Si), Sj)
                    for r in range(7):
                        Ji[r][d] = k * (ep[r] - em[r])
            if not self.fixed[j]:
                Jj = [[0.0] * 7 for _ in range(7)]
                for d in range(7):
                    ep = edge_error(M, Si, exp_apply(unit(d, DELTA), self.fix_scale, Sj))
                    em = edge_error(M, Si, exp_apply(unit(d, -DELTA), self.fix_scale, Sj))
                    for r in range(7):
                        Jj[r][d] = k * (ep[r] - em[r])
            E.append(e)
            J.append((Ji, Jj))
            chi_e.append(chi_of(e))

        def col_dot(X, a, Y, b):
            s = X[0][a] * Y[0][b]
            for r in range(1, 7):
                s = s + X[r][a] * Y[r][b]
            return s
        H, g = {}, {}
        for v in self.free:
            Hv, gv = [[0.0] * 7 for _ in range(7)], [0.0] * 7
            for ei, side in self.inc[v]:
                Jv = J[ei][side]
                for a in range(7):
                    for b in range(7):
                        Hv[a][b] = Hv[a][b] + col_dot(Jv, a, Jv, b)
                    t = Jv[0][a] * E[ei][0]
                    for r in range(1, 7):
                        t = t + Jv[r][a] * E[ei][r]
                    gv[a] = gv[a] + -t
            H[v], g[v] = Hv, gv
        A = {}
        for ei, (i, j) in enumerate(q["edges"]):
            if not self.fixed[i] and not self.fixed[j]:
                A[ei] = [[col_dot(J[ei][0], a, J[ei][1], b) for b in range(7)] for a in range(7)]
        return dict(E=E, J=J, H=H, g=g, A=A, chi=tree(list(enumerate(chi_e))))

    @staticmethod
    def factor(Hv, lam):
        """The Cholesky factor of Hv + lam I in solve6's loop order, or None when a pivot is not positive."""
        L = [[0.0] * 7 for _ in range(7)]
        ok = True
        for i in range(7):
            for j in range(i + 1):
                s = Hv[i][j] + lam if i == j else Hv[i][j]
                for k in range(j):
                    s = s - L[i][k] * L[j][k]
                if i == j:
                    ok = ok and s > 0
                    L[i][i] = _sqrt(s)
                else:
                    L[i][j] = _div(s, L[j][j])
        return L if ok else None

    @staticmethod
    def apply_factor(L, r):
        y, z = [0.0] * 7, [0.0] * 7
        for i in range(7):
            s = r[i]
            for k in range(i):
                s = s - L[i][k] * y[k]
            y[i] = _div(s, L[i][i])
        for i in range(6, -1, -1):
            s = y[i]
            for k in range(i + 1, 7):
                s = s - L[k][i] * z[k]
            z[i] = _div(s, L[i][i])
        return z

    def apply_system(self, lin, lam, p, v):
        Hv, pv = lin["H"][v], p[v]
        qv = []
        for a in range(7):
            s = (Hv[a][0] + lam if a == 0 else Hv[a][0]) * pv[0]
            for b in range(1, 7):
                s = s + (Hv[a][b] + lam if a == b else Hv[a][b]) * pv[b]
            qv.append(s)
        for ei, side in self.inc[v]:
            other = self.q["edges"][ei][1 - side]
            if self.fixed[other]:
                continue
            A, po = lin["A"][ei], p[other]
            for a in range(7):
                t = (A[0][a] if side else A[a][0]) * po[0]
                for b in range(1, 7):
                    t = t + (A[b][a] if side else A[a][b]) * po[b]
                qv[a] = qv[a] + t
        return qv

    def vsum(self, per_vertex):
        return tree([(v, per_vertex[v]) for v in self.free])

    def pcg(self, lin, lam, cap):
        """(failed, x, iterations) of G8."""
        L = {}
        failed = False
        for v in self.free:
            L[v] = self.factor(lin["H"][v], lam)
            failed = failed or L[v] is None
        if failed:
            self.paths.add("pivot_failed")
            return True, None, 0
        x = {v: [0.0] * 7 for v in self.free}
        r = {v: list(lin["g"][v]) for v in self.free}
        z = {v: self.apply_factor(L[v], r[v]) for v in self.free}
        p = {v: list(z[v]) for v in self.free}
        dn = self.vsum({v: dot7(r[v], z[v]) for v in self.free})
        d0, iters = dn, 0
        while dn > (TOL * TOL) * d0 and iters < cap:
            qq = {v: self.apply_system(lin, lam, p, v) for v in self.free}
            pq = self.vsum({v: dot7(p[v], qq[v]) for v in self.free})
            if not pq > 0.0 or not math.isfinite(pq):
                self.paths.add("pq_failed")
                return True, None, iters
            alpha = _div(dn, pq)
            for v in self.free:
                for k in range(7):
                    x[v][k] = x[v][k] + alpha * p[v][k]
                    r[v][k] = r[v][k] - alpha * qq[v][k]
                z[v] = self.apply_factor(L[v], r[v])
            dn2 = self.vsum({v: dot7(r[v], z[v]) for v in self.free})
            beta = _div(dn2, dn)
            for v in self.free:
                p[v] = [z[v][k] + beta * p[v][k] for k in range(7)]
            dn = dn2
            iters += 1
        if iters == 0:
            self.paths.add("pcg_zero_iterations")
        if iters == cap and dn > (TOL * TOL) * d0:
            self.paths.add("pcg_cap")
        return False, x, iters

    def run(self):
        """The result dict: V (list of (R, t, s)), lm (list of 3-lists), info (8 floats)."""
        q = self.q
        V = [state(*s) for s in q["V"]]
        info = [0.0] * 8
        if not self.free or self.n_e == 0:
            info[7] = 1.0
            self.paths.add("nothing_to_do")
            return self.finish(V, info)
        cap = q["pcg_max_iter"] if q["pcg_max_iter"] > 0 else 7 * len(self.free)
        lam, nu, chi, chi0, status = LAMBDA0, 2.0, 0.0, 0.0, 0.0
        it = trials = pcg_total = pcg_last = 0
        while it < q["num_iter"]:
            lin = self.linearize(V)
            if self.first is None:
                self.first = lin
            chi = lin["chi"]
            if it == 0:
                chi0 = chi
            if not math.isfinite(chi):
                status = 2.0
                self.paths.add("non_finite")
                break
            it += 1
            rho, qmax = 0.0, 0
            while True:
                failed, x, iters = self.pcg(lin, lam, cap)
                pcg_total += iters
                pcg_last = iters
                chi_new, scale = DBL_MAX, 0.0
                if not failed:
                    if self.first is lin and "x" not in lin:
                        lin["x"], lin["lambda"] = x, lam
                    Vt, sv = list(V), {}
                    for v in self.free:
                        s = 0.0
                        for k in range(7):
                            s = s + x[v][k] * (lam * x[v][k] + lin["g"][v][k])
                        sv[v] = s
                        Vt[v] = exp_apply(x[v], self.fix_scale, V[v])
                    scale = self.vsum(sv)
                    chi_new = tree([(ei, chi_of(edge_error(self.M[ei], Vt[i], Vt[j]))) for ei, (i, j) in enumerate(q["edges"])])
                rho = _div(chi - chi_new, scale + 1e-3)
                accepted = rho > 0 and math.isfinite(chi_new)
                self.trial_log.append((it, qmax, failed, accepted, chi, chi_new))
                self.paths.add(("accepted" if accepted else "rejected") + ("_first_trial" if qmax == 0 else "_later_trial"))
                if accepted:
                    xx = 2.0 * rho - 1.0
                    alpha = 1.0 - (xx * xx) * xx
                    alpha = 2.0 / 3.0 if 2.0 / 3.0 < alpha else alpha
                    lam = lam * (alpha if 1.0 / 3.0 < alpha else 1.0 / 3.0)
                    nu = 2.0
                    chi = chi_new
                    V = Vt
                else:
                    lam = lam * nu
                    nu = nu * 2.0
                qmax += 1
                trials += 1
                if not (rho < 0 and qmax < 10):
                    break
            if qmax == 10 or rho == 0:
                self.paths.add("ten_rejections" if qmax == 10 else "rho_zero")
                break
        else:
            self.paths.add("iteration_cap")
        info = [float(it), float(trials), chi0, chi, lam, float(pcg_total), float(pcg_last), status]
        return self.finish(V, info)

    def finish(self, V, info):
        q = self.q
        lm = []
        for r, p in zip(q["lm_ref"], q["lm_pos"]):
            if r < 0:
                lm.append(list(p))
                continue
            nc, S = state(*q["nc"][r]), V[r]
            w = [nc["s"] * dot3(nc["R"][3 * i], nc["R"][3 * i + 1], nc["R"][3 * i + 2], *p) + nc["t"][i] for i in range(3)]
            lm.append([S["s21"] * dot3(S["R"][i], S["R"][3 + i], S["R"][6 + i], *w) + S["t21"][i] for i in range(3)])
        return dict(V=[(list(S["R"]), list(S["t"]), S["s"]) for S in V], lm=lm, info=info)


def optimize(scene):
    return Optimizer(scene).run()
