"""The float64 restatement of crychic_render_sky (TEST INFRASTRUCTURE ONLY): numpy, written from the definition in
include/crychic_hip.h alone -- it imports nothing of tests/sky_ref, tests/sky_host or csrc.  Every step of the definition is restated
with exact operations (true division, sqrt, exp2, pow) in binary64; next to every quantity runs a bound on what binary32 evaluation
of the definition may differ from it by (DESIGN.md section 29 derives the rules), which decides what channels are marginal.

`mutate` names one deliberate misreading of the definition (MUTATIONS): the tests demand that each is caught.
`spacing` = "uniform" replaces the definition's quadratic sample spacing by a uniform one: tests/sky_quality.py measures both."""
import numpy as np

U = 2.0 ** -24                  # the unit roundoff of binary32
EXP2_REL = 4.0 * U              # det_exp2 against 2^z for an exact z: the degree-6 polynomial's 1.2e-7 plus its seven roundings
POW_REL = 3.0e-7                # pow_inv_gamma against x^(1/2.2)
LN2 = float(np.log(2.0))

RG, RT = 6360.0, 6420.0
HR, HM = 8.0, 1.2
BETA_R = np.array([5.8e-3, 13.5e-3, 33.1e-3], np.float32).astype(np.float64)
BETA_M = float(np.float32(21e-3))
G = 0.76
LOG2E = float(np.log2(np.e))

DEFAULTS = dict(sunDir=(0.0, 0.5, -0.8660254), altitude=0.002, sunIntensity=20.0, exposure=2.0, sunAngularRadius=0.02, groundAlbedo=0.3,
                viewSteps=16, sunSteps=8)
MUTATIONS = ("scale_heights_swapped", "extinction_1_0", "phase_without_1_plus_mu2", "planet_test_dropped", "half_step_dropped",
             "face_st_swapped", "ground_without_view_transmittance", "gamma_before_reinhard", "mie_phase_rayleigh_shape",
             "view_depth_without_half_sample")


def _f32(v):
    return float(np.float32(v))


class _Model:
    def __init__(self, params, mutate, spacing):
        p = dict(DEFAULTS, **(params or {}))
        self.mutate, self.spacing = mutate, spacing
        s = np.array([_f32(c) for c in p["sunDir"]], np.float64)
        self.S = s / np.sqrt((s * s).sum())
        alt = _f32(p["altitude"])
        self.r0 = RG + alt
        self.a0 = alt * (2.0 * RG + alt)
        self.cT = (RT - RG - alt) * (RT + RG + alt)
        self.r0Sy = self.r0 * self.S[1]
        self.Nv, self.Ns = int(p["viewSteps"]), int(p["sunSteps"])
        a2 = _f32(p["sunAngularRadius"]) ** 2
        self.cosDisc = 1.0 - a2 * (0.5 - a2 / 24.0)
        self.sunI, self.exposure = _f32(p["sunIntensity"]), _f32(p["exposure"])
        self.groundK = _f32(p["groundAlbedo"]) / np.pi * self.sunI
        self.hR, self.hM = (HM, HR) if mutate == "scale_heights_swapped" else (HR, HM)
        self.tauR = BETA_R * LOG2E
        self.tauM = (1.0 if mutate == "extinction_1_0" else 1.1) * BETA_M * LOG2E
        self.half = 0.0 if mutate == "half_step_dropped" else 0.5

    def samples(self, i, N, L, relL):
        """(t, dt, the relative error bound of both) of sample i of N over the segment of length L (known to relL)."""
        if self.spacing == "uniform":
            return L * ((i + self.half) / N), L / N, relL + 3 * U
        u = (i + self.half) / N
        return L * (u * u), L * ((2 * i + 1) / (N * N)), relL + 3 * U      # u, u u or (2 i + 1) invN2, L *: three roundings (invN: half an ulp more, inside)

    @staticmethod
    def height(q, eq):
        """(h, its absolute error bound) from q = r^2 - Rg^2 known to eq."""
        d = np.sqrt(q + RG * RG) + RG
        h = q / d
        return h, eq / d * (1.0 + np.abs(h) / d) + 4 * U * np.abs(h)       # the sum, the root, the sum, rcp, the product; d moves by eq / (2 r)

    def density(self, h, eh, H):
        """(2^(-h log2(e) / H), its relative error bound)."""
        z = -h * LOG2E / H
        return np.exp2(z), LN2 * (eh * LOG2E / H + 2 * U * np.abs(z)) + EXP2_REL        # the constant and the product round z

    @staticmethod
    def to_shell(c, b, ec, eb):
        """(the way to the shell, its relative error bound) from c = Rt^2 - r^2 >= 0 and b = P . dir, known to ec and eb."""
        sq = np.sqrt(b * b + c)
        esq = (2 * np.abs(b) * eb + ec + U * (b * b + c)) / (2 * sq) + U * sq
        up = b >= 0
        den = np.where(up, sq + b, 1.0)
        L = np.where(up, c / den, sq - b)
        rel_up = ec / np.maximum(c, 1e-300) + (esq + eb) / den + 3 * U
        rel_dn = (esq + eb) / np.maximum(sq - b, 1e-300) + U
        return L, np.where(up, rel_up, rel_dn)

    def sun_depth(self, q, bs, c, eq, ebs, ec):
        """(dR, dM, their absolute error bounds) of the sun march from the point (q, bs, c), known to (eq, ebs, ec)."""
        L, relL = self.to_shell(c, bs, ec, ebs)
        twob = bs + bs
        dR = dM = edR = edM = 0.0
        for j in range(self.Ns):
            s, ds, rs = self.samples(j, self.Ns, L, relL)
            qj = s * (s + twob) + q
            eqj = np.abs(s) * (rs * np.abs(s) + 2 * ebs + U * np.abs(s + twob)) + np.abs(s * (s + twob)) * rs + eq + U * np.abs(qj)
            h, eh = self.height(qj, eqj)
            for H, which in ((self.hR, 0), (self.hM, 1)):
                rho, rrho = self.density(h, eh, H)
                term = rho * ds
                if which == 0:
                    dR = dR + term
                    edR = edR + term * (rrho + rs) + U * dR
                else:
                    dM = dM + term
                    edM = edM + term * (rrho + rs) + U * dM
        return dR, dM, edR, edM

    def trans(self, dR, dM, edR, edM):
        """(the three channels' transmittance (n, 3), their relative error bounds)."""
        z = self.tauR[None, :] * np.asarray(dR)[:, None] + self.tauM * np.asarray(dM)[:, None]
        ez = self.tauR[None, :] * np.asarray(edR)[:, None] + self.tauM * np.asarray(edM)[:, None] + 3 * U * z
        return np.exp2(-z), LN2 * ez + EXP2_REL


def directions(dim, mutate=None):
    """The (6, dim, dim, 3) unnormalised directions of the texel centres."""
    c = (2.0 * np.arange(dim) + 1.0) / dim - 1.0
    s, t = np.meshgrid(c, c)            # s varies along x (the last axis), t along y
    if mutate == "face_st_swapped":
        s, t = t, s
    one = np.ones_like(s)
    faces = [(one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one)]
    return np.stack([np.stack(f, axis=-1) for f in faces])


def restate(dim, params=None, mutate=None, spacing="quadratic"):
    """(value, eps, risky): value (6, dim, dim, 3) float64, the three channels before rounding, in byte units (0 .. 255); eps, the
    same shape, the bound on what binary32 evaluation moves value by; risky (6, dim, dim) bool, texels whose ground test, disc test
    or any planet test falls within its error bound of equality (their value follows the float64 decision)."""
    assert mutate is None or mutate in MUTATIONS
    with np.errstate(all="ignore"):         # lanes whose result is not selected (a blocked sample's sun march) may overflow
        return _restate(dim, params, mutate, spacing)


def _restate(dim, params, mutate, spacing):
    m = _Model(params, mutate, spacing)
    d = directions(dim, mutate).reshape(-1, 3)
    n = d.shape[0]
    v = d / np.sqrt((d * d).sum(axis=1))[:, None]
    ev = 5 * U                                          # every component of v, |v| <= 1: s or t, the dot product, the root, rcp, the product
    mu = v @ m.S
    emu = 3 * ev + 3 * U
    b = m.r0 * v[:, 1]
    eb = m.r0 * (ev + U)
    twob = 2 * b
    ea0 = U * m.a0
    dg = b * b - m.a0
    edg = 2 * np.abs(b) * eb + ea0 + U * np.abs(dg) + U * b * b
    ground = (b < 0) & (dg >= 0)
    risky = (np.abs(b) <= eb) | ((b < 0) & (np.abs(dg) <= edg))
    sqg = np.sqrt(np.maximum(dg, 0.0))
    tG = m.a0 / np.maximum(sqg - b, 1e-300)
    relG = U + (edg / np.maximum(2 * sqg, 1e-300) + eb) / np.maximum(sqg - b, 1e-300) + 3 * U
    relG = np.where(m.a0 == 0.0, 0.0, np.minimum(relG, 1.0))
    tS, relS = m.to_shell(m.cT, b, U * m.cT, eb)
    tEnd = np.where(ground, tG, tS)
    relEnd = np.where(ground, relG, relS)

    vR = np.zeros(n); vM = np.zeros(n); evR = np.zeros(n); evM = np.zeros(n)
    sR = np.zeros((n, 3)); sM = np.zeros((n, 3)); esR = np.zeros((n, 3)); esM = np.zeros((n, 3))
    for i in range(m.Nv):
        t, dt, rt = m.samples(i, m.Nv, tEnd, relEnd)
        w = t * (t + twob)
        ew = np.abs(t) * (rt * np.abs(t) + 2 * eb + U * np.abs(t + twob)) + np.abs(w) * (rt + U)
        q = m.a0 + w
        eq = ew + ea0 + U * np.abs(q)
        h, eh = m.height(q, eq)
        dR_, rR = m.density(h, eh, m.hR)
        dM_, rM = m.density(h, eh, m.hM)
        rhoR, rhoM = dR_ * dt, dM_ * dt
        rR, rM = rR + rt + U, rM + rt + U
        if mutate == "view_depth_without_half_sample":
            mR, mM = vR, vM
        else:
            mR, mM = vR + 0.5 * rhoR, vM + 0.5 * rhoM
        emR, emM = evR + 0.5 * rhoR * rR + U * mR, evM + 0.5 * rhoM * rM + U * mM
        vR, vM = vR + rhoR, vM + rhoM
        evR, evM = evR + rhoR * rR + U * vR, evM + rhoM * rM + U * vM
        bs = t * mu + m.r0Sy
        ebs = np.abs(t) * (emu + rt * np.abs(mu)) + U * np.abs(m.r0Sy) + U * np.abs(bs)
        disc2 = bs * bs - q
        edisc2 = 2 * np.abs(bs) * ebs + eq + U * np.abs(disc2) + U * bs * bs
        blocked = (bs < 0) & (disc2 >= 0)
        risky |= (dt > 0) & ((np.abs(bs) <= ebs) | ((bs < 0) & (np.abs(disc2) <= edisc2)))      # a sample of no length adds nothing either way
        if mutate == "planet_test_dropped":
            blocked = np.zeros(n, bool)
        c = np.maximum(m.cT - w, 0.0)
        dR, dM, edR, edM = m.sun_depth(q, bs, c, eq, ebs, ew + 2 * U * m.cT)
        T, rT = m.trans(mR + dR, mM + dM, emR + edR + U * (mR + dR), emM + edM + U * (mM + dM))
        lit = (~blocked)[:, None]
        termR, termM = T * rhoR[:, None], T * rhoM[:, None]
        sR = np.where(lit, sR + termR, sR)
        sM = np.where(lit, sM + termM, sM)
        esR = np.where(lit, esR + termR * (rT + rR[:, None] + U) + U * sR, esR)
        esM = np.where(lit, esM + termM * (rT + rM[:, None] + U) + U * sM, esM)

    m1 = np.ones(n) if mutate == "phase_without_1_plus_mu2" else 1.0 + mu * mu
    phR = 3.0 / (16.0 * np.pi) * m1
    xg = 1.0 + G * G - 2.0 * G * mu
    if mutate == "mie_phase_rayleigh_shape":
        phM = phR
    else:
        phM = 3.0 * (1.0 - G * G) / (8.0 * np.pi * (2.0 + G * G)) * m1 / (xg * np.sqrt(xg))
    rphR = np.full(n, 2 * emu + 3 * U)                                      # m1 >= 1 moves by 2 |mu| emu
    rphM = rphR + 2.5 * (1.52 * emu + U * xg) / xg + 5 * U           # xg^(3/2): the product, the root, rcp, two more products
    aR = phR[:, None] * BETA_R[None, :] * sR
    aM = phM[:, None] * BETA_M * sM
    L = m.sunI * (aR + aM)
    eL = m.sunI * (aR * (rphR[:, None] + 2 * U) + phR[:, None] * BETA_R[None, :] * esR
                   + aM * (rphM[:, None] + 3 * U) + phM[:, None] * BETA_M * esM) + 2 * U * L

    disc = ~ground & (mu >= m.cosDisc)
    risky |= ~ground & (np.abs(mu - m.cosDisc) <= emu + U)
    w = tEnd * (tEnd + twob)
    q = np.maximum(m.a0 + w, 0.0)
    ew = np.abs(tEnd) * (relEnd * np.abs(tEnd) + 2 * eb + U * np.abs(tEnd + twob)) + np.abs(w) * (relEnd + U)
    eq = ew + ea0 + U * q
    bs = tEnd * mu + m.r0Sy
    ebs = np.abs(tEnd) * (emu + relEnd * np.abs(mu)) + U * np.abs(m.r0Sy) + U * np.abs(bs)
    sunlit = ground & (bs > 0)
    Tv, rTv = m.trans(vR, vM, evR, evM)
    bsl = np.where(sunlit, bs, 1.0)                                   # a stand-in where the march is not used
    dR, dM, edR, edM = m.sun_depth(q, bsl, np.maximum(m.cT - w, 0.0), eq, ebs, ew + 2 * U * m.cT)
    Tg, rTg = m.trans(dR, dM, edR, edM)
    cosG = bs / RG
    g = m.groundK * cosG[:, None] * Tg
    rg = rTg + (ebs / np.maximum(np.abs(bs), 1e-300))[:, None] + 5 * U
    if mutate != "ground_without_view_transmittance":
        g = g * Tv
        rg = rg + rTv
    L = np.where(sunlit[:, None], L + g, L)
    eL = np.where(sunlit[:, None], eL + g * rg + U * L, eL)
    # the ground term is continuous where the sun stands on the ground point's horizon: deciding bs > 0 the other way adds or drops
    # at most the term of a sun ebs above it
    eL = np.where((ground & (np.abs(bs) <= ebs))[:, None], eL + m.groundK * (ebs / RG)[:, None], eL)
    sd = m.sunI * Tv
    L = np.where(disc[:, None], L + sd, L)
    eL = np.where(disc[:, None], eL + sd * (rTv + U) + U * L, eL)

    e = L * m.exposure
    ee = eL * m.exposure + U * e
    if mutate == "gamma_before_reinhard":
        y = e ** (1.0 / 2.2)
        tm = y / (1.0 + y)
    else:
        tm = (e / (1.0 + e)) ** (1.0 / 2.2)
    # the slope of tm in e: tm / (2.2 e (1 + e)); the tone map's own roundings: the sum, rcp and the product (each moves x / (1 + x)
    # by at most U of it, tm by 1 / 2.2 of that), pow_inv_gamma, and the fma of the quantisation
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = np.where(e > 0, tm / (2.2 * np.maximum(e, 1e-300) * (1.0 + e)), 0.0)
    value = np.minimum(tm, 1.0) * 255.0
    eps = 255.0 * (slope * ee + tm * (3 * U / 2.2 + POW_REL)) + 256.0 * U
    return value.reshape(6, dim, dim, 3), eps.reshape(6, dim, dim, 3), risky.reshape(6, dim, dim)


def classify(value, eps, risky):
    """(byte, marginal): byte (.., 3) uint8, floor(value + 0.5); marginal (.., 3) bool: value + 0.5 lies within eps of an integer, or
    the texel is risky."""
    x = value + 0.5
    byte = np.floor(x)
    marginal = (np.abs(x - np.round(x)) <= eps) | risky[..., None]
    return np.clip(byte, 0, 255).astype(np.uint8), marginal
