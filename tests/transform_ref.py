"""Sequential restatement of optimize::transform_optimizer::optimize as DESIGN.md 3.11 fixes it (rules 1 to 8): one match after the other, one
trial after the other. Pure Python on purpose: a Python float is an IEEE f64 and every operation below rounds once, so the results are the
bits the rules ask for. No numpy in the arithmetic; imports nothing of the product. The three deterministic functions of rule 3 are restated
here from exact fractions (the oracle library cannot evaluate them); asin / atan2 of the equirectangular projection are tests/sim3_ref.py's.

A problem is a dict: p1, p2 (lists of 3-tuples), obs1, obs2 (lists of 2-tuples), w1, w2 (lists of floats that hold f32 values), cam_1, cam_2
(reference camera dicts), R (9, row-major), t (3), s: the initial Sim3_12."""
import math
from fractions import Fraction
from math import factorial

from sim3_ref import _div, _sqrt, bits, dot3, f32, project  # noqa: F401

EPS, DELTA, DBL_MAX = 1e-5, 1e-9, 1.7976931348623157e308
NAN = float("nan")
S_K = [float(Fraction((-1) ** k, factorial(2 * k + 1))) for k in range(9)]
C_K = [float(Fraction((-1) ** k, factorial(2 * k))) for k in range(9)]
E_K = [float(Fraction(1, factorial(k))) for k in range(15)]
PI_O_4 = math.pi / 4.0


# ---- rule 3
def _sincos(x):
    if not abs(x) <= 1048576.0:
        return NAN, NAN
    m = 0
    while abs(x) > PI_O_4:
        x = x * 0.5
        m += 1
    z = x * x
    p = S_K[8]
    for k in range(7, 0, -1):
        p = S_K[k] + z * p
    s = x + x * (z * p)
    p = C_K[8]
    for k in range(7, 1, -1):
        p = C_K[k] + z * p
    c = (1.0 - 0.5 * z) + z * (z * p)
    for _ in range(m):
        s, c = 2.0 * (s * c), 1.0 - 2.0 * (s * s)
    return s, c


def det_sin(x):
    return _sincos(x)[0]


def det_cos(x):
    return _sincos(x)[1]


def det_exp(x):
    if not abs(x) <= 32.0:
        return NAN
    m = 0
    while abs(x) > 0.3125:
        x = x * 0.5
        m += 1
    p = E_K[14]
    for k in range(13, 1, -1):
        p = E_K[k] + x * p
    e = 1.0 + (x + x * (x * p))
    for _ in range(m):
        e = e * e
    return e


# ---- rules 1 and 2
def with_inverse(R, t, s):
    s21 = _div(1.0, s)
    return dict(R=list(R), t=list(t), s=s, s21=s21, t21=[(-s21) * dot3(R[r], R[3 + r], R[6 + r], *t) for r in range(3)])


def exp_parts(u, fix_scale):
    """(Re, te, se, branch) of exp(u); branch names which of rule 2's four the coefficients took."""
    w0, w1, w2 = u[0], u[1], u[2]
    sigma = 0.0 if fix_scale else u[6]
    theta = _sqrt(dot3(w0, w1, w2, w0, w1, w2))
    Om = [0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0]
    Om2 = [(Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j]) + Om[3 * i + 2] * Om[6 + j] for i in range(3) for j in range(3)]
    se = det_exp(sigma)
    sn, cs = _sincos(theta)
    th2 = theta * theta
    small_t, small_s = theta < EPS, abs(sigma) < EPS
    I = [1.0 if k % 4 == 0 else 0.0 for k in range(9)]
    if small_t:
        Re = [(I[k] + Om[k]) + Om2[k] / 2.0 for k in range(9)]
    else:
        ka, kb = _div(sn, theta), _div(1.0 - cs, th2)
        Re = [(I[k] + ka * Om[k]) + kb * Om2[k] for k in range(9)]
    if small_s:
        C = 1.0
        if small_t:
            A, B = 0.5, 1.0 / 6.0
        else:
            A, B = _div(1.0 - cs, th2), _div(theta - sn, th2 * theta)
    else:
        C = _div(se - 1.0, sigma)
        sg2 = sigma * sigma
        if small_t:
            A = _div((sigma - 1.0) * se + 1.0, sg2)
            B = _div((0.5 * sg2 - sigma + 1.0) * se - 1.0, sg2 * sigma)
        else:
            a, b, c = se * sn, se * cs, th2 + sg2
            A = _div(a * sigma + (1.0 - b) * theta, theta * c)
            B = _div(C - _div((b - 1.0) * sigma + a * theta, c), th2)
    W = [(A * Om[k] + B * Om2[k]) + C * I[k] for k in range(9)]
    te = [dot3(W[3 * i], W[3 * i + 1], W[3 * i + 2], u[3], u[4], u[5]) for i in range(3)]
    return Re, te, se, ("small" if small_t else "large") + "_theta_" + ("small" if small_s else "large") + "_sigma"


def exp_apply(u, fix_scale, S):
    Re, te, se, _ = exp_parts(u, fix_scale)
    R = [(Re[3 * i] * S["R"][j] + Re[3 * i + 1] * S["R"][3 + j]) + Re[3 * i + 2] * S["R"][6 + j] for i in range(3) for j in range(3)]
    t = [se * dot3(Re[3 * i], Re[3 * i + 1], Re[3 * i + 2], *S["t"]) + te[i] for i in range(3)]
    return with_inverse(R, t, se * S["s"])


# ---- rule 4
def edges_of(prob, S, i):
    p1, p2, R = prob["p1"][i], prob["p2"][i], S["R"]
    x1 = S["s"] * dot3(R[0], R[1], R[2], *p2) + S["t"][0]
    y1 = S["s"] * dot3(R[3], R[4], R[5], *p2) + S["t"][1]
    z1 = S["s"] * dot3(R[6], R[7], R[8], *p2) + S["t"][2]
    x2 = S["s21"] * dot3(R[0], R[3], R[6], *p1) + S["t21"][0]
    y2 = S["s21"] * dot3(R[1], R[4], R[7], *p1) + S["t21"][1]
    z2 = S["s21"] * dot3(R[2], R[5], R[8], *p1) + S["t21"][2]
    u, v = project(prob["cam_1"], x1, y1, z1)
    e1 = (prob["obs1"][i][0] - u, prob["obs1"][i][1] - v)
    u, v = project(prob["cam_2"], x2, y2, z2)
    e2 = (prob["obs2"][i][0] - u, prob["obs2"][i][1] - v)
    return e1, e2, z1, z2


def chi_of(e, w):
    return w * (e[0] * e[0] + e[1] * e[1])


class Optimizer:
    """One run of rules 5 to 8 with what the tests ask about it: margins, paths, the info record."""

    def __init__(self, prob, fix_scale, chi_sq=10.0, num_iter=10):
        self.prob, self.fix_scale, self.num_iter = prob, bool(fix_scale), int(num_iter)
        self.chi_sq = f32(chi_sq)
        self.delta = f32(math.sqrt(self.chi_sq))    # (double)sqrtf(chi_sq): the square root of an f32 rounded to f32 is sqrtf's result
        self.delta_sq = self.delta * self.delta
        self.n = len(prob["p1"])
        self.huber_margin = float("inf")            # the smallest |chi - delta^2| / delta^2 over every evaluation
        self.gate_margin = float("inf")             # the smallest |chi - chi_sq| / chi_sq over every classified edge
        self.paths = set()
        self.trial_log = []

    def huber(self, chi):
        if math.isfinite(chi):
            self.huber_margin = min(self.huber_margin, abs(chi - self.delta_sq) / self.delta_sq)
        if chi > self.delta_sq:
            r = _sqrt(chi)
            return 2.0 * r * self.delta - self.delta_sq, _div(self.delta, r)
        return chi, 1.0

    def robust_chi_of(self, S, i):
        e1, e2, _, _ = edges_of(self.prob, S, i)
        return self.huber(chi_of(e1, self.prob["w1"][i]))[0] + self.huber(chi_of(e2, self.prob["w2"][i]))[0]

    def is_inlier(self, S, i):
        q = self.prob
        e1, e2, z1, z2 = edges_of(q, S, i)
        c1, c2 = chi_of(e1, q["w1"][i]), chi_of(e2, q["w2"][i])
        for c in (c1, c2):
            if math.isfinite(c):
                self.gate_margin = min(self.gate_margin, abs(c - self.chi_sq) / self.chi_sq)
        ok = c1 <= self.chi_sq and c2 <= self.chi_sq
        if q["cam_1"]["model"] == 0:
            ok = ok and q["p1"][i][2] > 0.0 and z1 > 0.0
        if q["cam_2"]["model"] == 0:
            ok = ok and q["p2"][i][2] > 0.0 and z2 > 0.0
        return ok

    def tree(self, per_match, K, outlier):
        """Rule 6's sum order: partial j of 64 takes the matches j, j + 64, ... from 0.0; then part[j] += part[j + d], d = 32 .. 1."""
        part = [[0.0] * K for _ in range(64)]
        for j in range(64):
            for i in range(j, self.n, 64):
                if not outlier[i]:
                    per_match(i, part[j])
        d = 32
        while d:
            for j in range(d):
                for k in range(K):
                    part[j][k] = part[j][k] + part[j + d][k]
            d >>= 1
        return part[0]

    def accumulate(self, S, pert, i, acc):
        q = self.prob
        k = 1.0 / (2.0 * DELTA)
        e1, e2, _, _ = edges_of(q, S, i)
        J1, J2 = [[0.0] * 7, [0.0] * 7], [[0.0] * 7, [0.0] * 7]
        for d in range(7):
            p1, p2, _, _ = edges_of(q, pert[2 * d], i)
            m1, m2, _, _ = edges_of(q, pert[2 * d + 1], i)
            J1[0][d], J1[1][d] = k * (p1[0] - m1[0]), k * (p1[1] - m1[1])
            J2[0][d], J2[1][d] = k * (p2[0] - m2[0]), k * (p2[1] - m2[1])
        r01, r11 = self.huber(chi_of(e1, q["w1"][i]))
        r02, r12 = self.huber(chi_of(e2, q["w2"][i]))
        W1, W2 = r11 * q["w1"][i], r12 * q["w2"][i]
        idx = 0
        for a in range(7):
            for b in range(a, 7):
                acc[idx] = acc[idx] + (W1 * (J1[0][a] * J1[0][b] + J1[1][a] * J1[1][b]) + W2 * (J2[0][a] * J2[0][b] + J2[1][a] * J2[1][b]))
                idx += 1
        for a in range(7):
            acc[28 + a] = acc[28 + a] + -(W1 * (J1[0][a] * e1[0] + J1[1][a] * e1[1]) + W2 * (J2[0][a] * e2[0] + J2[1][a] * e2[1]))
        acc[35] = acc[35] + (r01 + r02)

    @staticmethod
    def solve7(sums, lam):
        """(ok, dx): the 7 x 7 Cholesky in solve6's loop order."""
        H = [[0.0] * 7 for _ in range(7)]
        idx = 0
        for a in range(7):
            for b in range(a, 7):
                H[a][b] = H[b][a] = sums[idx]
                idx += 1
        L = [[0.0] * 7 for _ in range(7)]
        for i in range(7):
            for j in range(i + 1):
                s = H[i][j] + (lam if i == j else 0.0)
                for k in range(j):
                    s = s - L[i][k] * L[j][k]
                if i == j:
                    if not s > 0:
                        return False, None
                    L[i][i] = math.sqrt(s)
                else:
                    L[i][j] = _div(s, L[j][j])
        y, dx = [0.0] * 7, [0.0] * 7
        for i in range(7):
            s = sums[28 + i]
            for k in range(i):
                s = s - L[i][k] * y[k]
            y[i] = _div(s, L[i][i])
        for i in range(6, -1, -1):
            s = y[i]
            for k in range(i + 1, 7):
                s = s - L[k][i] * dx[k]
            dx[i] = _div(s, L[i][i])
        return True, dx

    def run(self):
        """The result dict: num_inliers, R, t, s, flags (1 = outlier), info (8 floats)."""
        q, n = self.prob, self.n
        S_in = with_inverse(q["R"], q["t"], q["s"])
        S = S_in
        outlier = [0] * n
        info = [0.0] * 8
        survivors, iters = n, 5
        for rnd in range(2):
            Serr = S
            lam, nu, current_chi = 0.0, 2.0, 0.0
            it = trials = 0
            accepted_last = None
            while it < iters:
                Serr = S
                pert = []
                for d in range(7):
                    for sign in (DELTA, -DELTA):
                        pert.append(exp_apply([sign if k == d else 0.0 for k in range(7)], self.fix_scale, S))
                sums = self.tree(lambda i, acc: self.accumulate(S, pert, i, acc), 36, outlier)
                current_chi = sums[35]
                if it == 0:
                    md, idx = 0.0, 0
                    for j in range(7):
                        a = abs(sums[idx])
                        md = md if a < md else a
                        idx += 7 - j
                    lam, nu = 1e-5 * md, 2.0
                it += 1
                rho, qmax = 0.0, 0
                while True:
                    ok, dx = self.solve7(sums, lam)
                    Sn, temp_chi, scale = S, DBL_MAX, 0.0
                    if ok:
                        Sn = exp_apply(dx, self.fix_scale, S)
                        self.paths.add("sigma_small" if abs(0.0 if self.fix_scale else dx[6]) < EPS else "sigma_large")
                        state = Sn

                        def add_chi(i, acc):
                            acc[0] = acc[0] + self.robust_chi_of(state, i)
                        temp_chi = self.tree(add_chi, 1, outlier)[0]
                        Serr = Sn
                        for j in range(7):
                            scale = scale + dx[j] * (lam * dx[j] + sums[28 + j])
                    rho = _div(current_chi - temp_chi, scale + 1e-3)
                    accepted_last = rho > 0 and math.isfinite(temp_chi)
                    self.trial_log.append((rnd, it, qmax, ok, accepted_last))
                    if accepted_last:
                        x = 2.0 * rho - 1.0
                        alpha = 1.0 - (x * x) * x
                        alpha = 2.0 / 3.0 if 2.0 / 3.0 < alpha else alpha
                        lam = lam * (alpha if 1.0 / 3.0 < alpha else 1.0 / 3.0)
                        nu = 2.0
                        current_chi = temp_chi
                        S = Sn
                    else:
                        lam = lam * nu
                        nu = nu * 2.0
                    qmax += 1
                    trials += 1
                    if not (rho < 0 and qmax < 10):
                        break
                if qmax == 10 or rho == 0:
                    break
            info[4 * rnd], info[4 * rnd + 1], info[4 * rnd + 2], info[7] = float(it), float(trials), current_chi, lam
            if accepted_last is not None:
                self.paths.add("round%d_ends_%s" % (rnd + 1, "accepted" if accepted_last else "rejected"))
            Sc = Serr if rnd == 0 else S
            count = 0
            for i in range(n):
                if not outlier[i]:
                    inl = self.is_inlier(Sc, i)
                    outlier[i] = 0 if inl else 1
                    count += 1 if inl else 0
            before, survivors = survivors, count
            if rnd == 0:
                info[3] = float(n - survivors)
                if survivors < 10:
                    self.paths.add("too_few_survivors")
                    return dict(num_inliers=0, R=list(q["R"]), t=list(q["t"]), s=q["s"], flags=outlier, info=info)
                iters = self.num_iter if survivors < before else 5
                self.paths.add("round2_num_iter" if survivors < before else "round2_five")
        return dict(num_inliers=survivors, R=S["R"], t=S["t"], s=S["s"], flags=outlier, info=info)


def optimize(prob, fix_scale, chi_sq=10.0, num_iter=10):
    return Optimizer(prob, fix_scale, chi_sq, num_iter).run()
