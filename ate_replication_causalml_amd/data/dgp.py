"""Synthetic data with the tutorial's schema.

The reference reads the Gerber-Green-Larimer social-pressure CSV
(``ate_replication.Rmd:32-34``), which is not shipped (``.gitignore:6``).
This module generates data with the same schema: 15 continuous covariates
(standardised with ``scale()``, ``ate_replication.Rmd:72-74``), 6 binary
covariates, binary outcome ``Y`` (``outcome_voted``) and binary treatment ``W``
(``treat_neighbors``), in the reference column order (cts, bin, Y, W;
``ate_replication.Rmd:90-93``).

Every draw is a Philox function of (seed, column stream, row index), so the
same rows can be produced on the host (this file) or directly in HBM by the
``dgp_fill`` HIP kernel for the scaled configs (N up to 1e8, p up to 2000),
without ever materialising the panel on the host.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ..parallel import rng

CTS_NAMES = [
    "yob", "city", "hh_size", "totalpopulation_estimate", "percent_male", "median_age",
    "percent_62yearsandover", "percent_white", "percent_black", "percent_asian",
    "median_income", "employ_20to64", "highschool", "bach_orhigher",
    "percent_hispanicorlatino",
]  # ate_replication.Rmd:49-55
BIN_NAMES = ["sex", "g2000", "g2002", "p2000", "p2002", "p2004"]  # ate_replication.Rmd:56
COVARIATES = CTS_NAMES + BIN_NAMES  # ate_replication.Rmd:57

S_CTS = 0           # streams 0..14: continuous covariates
S_FACTOR = 40       # shared census-block factor for the neighbourhood covariates
S_LATENT = 41       # latent propensity to vote
S_HIST = 50         # 50..54 vote history g2000..p2004
S_SEX = 60
S_W = 61
S_Y = 62
S_EXTRA = 100       # 100.. extra nuisance columns for scaled configs


@dataclass(frozen=True)
class DgpParams:
    """Constants of the latent-voter model: 15 N(0,1) continuous
    covariates (3 individual, 12 loading on a census-block factor), latent = N(0,1) +
    yob_latent * yob, vote history k = 1[N(0,1) + hist_latent * latent > hist_thresh[k]]
    (g2000, g2002, p2000, p2002, p2004), sex ~ Bern(0.5), W ~ Bern(p_treat) (the RCT),
    Y ~ Bern(sigmoid(intercept + b_hist' history + b_latent * latent + tau_logit * W))."""
    intercept: float = -1.4
    b_hist: tuple = (0.3, 0.3, 0.3, 0.3, 0.3)
    b_latent: float = 0.2
    tau_logit: float = 0.45
    p_treat: float = 1.0 / 6.0
    hist_thresh: tuple = (0.6, 0.6, 0.6, 0.6, 0.6)
    hist_latent: float = 0.5
    yob_latent: float = 0.3
    factor_load: float = 0.6

    def device_block(self) -> np.ndarray:
        """The float64[18] parameter block of csrc/dgp.hip (load_params: the selection
        rule's parameters used at full precision, the rest rounded to fp32 there)."""
        fl = self.factor_load
        return np.array([self.intercept, *self.b_hist, self.b_latent, self.tau_logit,
                         self.p_treat, *self.hist_thresh, self.hist_latent, self.yob_latent,
                         fl, np.sqrt(1 - fl ** 2)], dtype=np.float64)


# The scaled-config panels (data/device_dgp.synthetic_panel, the bench) and the HIP
# generator csrc/dgp.hip: the survey's scratch constants (one history threshold).
PANEL = DgpParams()
# The tutorial replication (make_tutorial_data): recalibrated to the published run
# (ate_replication.md:118 and the three plots) -- vote-history marginals
# like the real file's (general elections ~0.8, primaries ~0.3-0.45) so the selection
# transform drops ~41,062 of 50,000 rows, and a baseline turnout / effect profile under
# which the published ordering holds: oracle ~0.096, naive ~0, logistic-PS IPW below the
# oracle, LASSO-PS IPW below that, Double ML in [0.03, 0.08] (tools/dgp_calibrate.py,
# tests/test_dgp_calibration.py).
# Thresholds: -Phi^-1(marginal) * sd(history score), marginals (0.85, 0.80, 0.25, 0.40,
# 0.40), sd = sqrt(1 + 0.4^2 (1 + 0.3^2)). At n = 50,000, seed 1991 (CPU reference path,
# tools/dgp_calibrate.py): 40,584 rows dropped (published 41,062), oracle 0.0945 (0.0961),
# naive -0.0012 (0.0028), OLS 0.0888 (0.0777), IPW logistic PS 0.0694 (0.0637), IPW
# LASSO PS 0.0117 (0.0110), Double ML (200 trees) 0.0533 (0.0524).
TUTORIAL = DgpParams(intercept=-1.8, b_hist=(0.35, 0.35, 0.35, 0.35, 0.35), b_latent=0.35,
                     tau_logit=0.4, p_treat=1.0 / 6.0,
                     hist_thresh=(-1.1232, -0.9121, 0.7309, 0.2746, 0.2746), hist_latent=0.4)

# legacy names (the panel model)
INTERCEPT, B_LATENT, TAU_LOGIT, P_TREAT = PANEL.intercept, PANEL.b_latent, PANEL.tau_logit, \
    PANEL.p_treat
B_HIST, HIST_THRESH = PANEL.b_hist[0], PANEL.hist_thresh[0]
HIST_LATENT, YOB_LATENT, FACTOR_LOAD = PANEL.hist_latent, PANEL.yob_latent, PANEL.factor_load


def _normal(seed, stream, idx):
    return rng.normal_pair(seed, rng.P_DGP, stream, idx)[0]


def _uniform(seed, stream, idx):
    return rng.uniform(seed, rng.P_DGP, stream, idx)


@dataclass
class TutorialData:
    X: np.ndarray          # (n, p) float64, columns named by ``names``
    W: np.ndarray          # (n,) float64 in {0,1}
    Y: np.ndarray          # (n,) float64 in {0,1}
    names: list
    tau_true: float        # population ATE on the probability scale (MC of the DGP)

    @property
    def n(self):
        return self.X.shape[0]

    def to_frame(self):
        import pandas as pd
        df = pd.DataFrame(self.X, columns=self.names)
        df["Y"] = self.Y
        df["W"] = self.W
        return df


def raw_columns(n: int, seed: int, p_extra: int = 0, row_offset: int = 0,
                params: DgpParams = PANEL, idx=None):
    """Unscaled draws for rows [row_offset, row_offset+n), or for the generated-row ids
    ``idx`` (the model of the HIP generator csrc/dgp.hip, row for row; float64 here, float32
    on the device)."""
    P = params
    idx = np.arange(row_offset, row_offset + n, dtype=np.uint64) if idx is None else \
        np.asarray(idx, dtype=np.uint64)
    n = len(idx)
    f = _normal(seed, S_FACTOR, idx)
    fl = P.factor_load
    cts = np.empty((n, 15))
    for j in range(15):
        z = _normal(seed, S_CTS + j, idx)
        cts[:, j] = z if j < 3 else fl * f + np.sqrt(1 - fl ** 2) * z
    latent = _normal(seed, S_LATENT, idx) + P.yob_latent * cts[:, 0]
    hist = np.empty((n, 5))
    for k in range(5):
        hist[:, k] = (_normal(seed, S_HIST + k, idx) + P.hist_latent * latent > P.hist_thresh[k])
    sex = (_uniform(seed, S_SEX, idx) < 0.5).astype(np.float64)
    W = (_uniform(seed, S_W, idx) < P.p_treat).astype(np.float64)
    eta = P.intercept + hist @ np.asarray(P.b_hist, dtype=np.float64) + P.b_latent * latent
    Y = (_uniform(seed, S_Y, idx) < 1.0 / (1.0 + np.exp(-(eta + P.tau_logit * W)))).astype(
        np.float64)
    tau_i = 1 / (1 + np.exp(-(eta + P.tau_logit))) - 1 / (1 + np.exp(-eta))
    extra = np.empty((n, p_extra))
    for j in range(p_extra):
        z = _normal(seed, S_EXTRA + j, idx)
        if j % 4 == 3:   # every 4th extra column is binary
            extra[:, j] = (z > 0).astype(np.float64)
        else:
            extra[:, j] = fl * f + np.sqrt(1 - fl ** 2) * z
    return cts, np.column_stack([sex, hist]), extra, W, Y, tau_i


def selection_flags(seed: int, idx, params: DgpParams, compat: str = "reference") -> np.ndarray:
    """Host twin of csrc/dgp.hip sel_flag for generated rows ``idx``: 1 treated candidate,
    2 control candidate, 0 neither (ate_replication.Rmd:103-110 on the population-
    standardised yob / city, i.e. +-2 on the raw N(0,1) draws; quirk Q17 under
    compat="reference")."""
    P = params
    idx = np.asarray(idx, dtype=np.uint64)
    yob = _normal(seed, S_CTS + 0, idx)
    city = _normal(seed, S_CTS + 1, idx)
    latent = _normal(seed, S_LATENT, idx) + P.yob_latent * yob
    h = [(_normal(seed, S_HIST + k, idx) + P.hist_latent * latent > P.hist_thresh[k])
         for k in range(5)]
    W = _uniform(seed, S_W, idx) < P.p_treat
    last = h[3] if compat == "reference" else h[4]
    dt = h[0] | h[1] | h[2] | h[3] | last | (city > 2) | (yob > 2)
    dc = ~h[0] | ~h[1] | ~h[2] | ~h[3] | ~h[4] | (city < -2) | (yob < -2)
    return np.where(W, np.where(dt, 1, 0), np.where(dc, 2, 0)).astype(np.uint8)


def r_scale(a: np.ndarray) -> np.ndarray:
    """R ``scale()``: centre and divide by the sample SD (n-1 denominator)."""
    m = a.mean(0)
    s = a.std(0, ddof=1)
    s = np.where(s > 0, s, 1.0)
    return (a - m) / s


def make_tutorial_data(n: int = 50_000, seed: int = 1991, p_extra: int = 0,
                       params: DgpParams = TUTORIAL) -> TutorialData:
    """The ``df`` of ``ate_replication.Rmd:89-94`` (scaled cts + binary + Y + W)."""
    cts, binc, extra, W, Y, tau_i = raw_columns(n, seed, p_extra, params=params)
    cts = r_scale(cts)
    names = list(COVARIATES)
    blocks = [cts, binc]
    if p_extra:
        ex = extra.copy()
        cont = [j for j in range(p_extra) if j % 4 != 3]
        ex[:, cont] = r_scale(ex[:, cont])
        blocks.append(ex)
        names += [f"x_extra{j}" for j in range(p_extra)]
    X = np.column_stack(blocks)
    return TutorialData(X=X, W=W, Y=Y, names=names, tau_true=float(tau_i.mean()))


S_Z = 70            # LATE data: the instrument (the treatment assigned)
S_TYPE = 71         # LATE data: the latent compliance type
S_YL = 72           # LATE data: the outcome


@dataclass
class LateData:
    X: np.ndarray          # (n, p) float64, the tutorial's covariates
    Y: np.ndarray          # (n,) float64 in {0,1}
    D: np.ndarray          # (n,) float64 in {0,1}: the treatment taken
    Z: np.ndarray          # (n,) float64 in {0,1}: the instrument (the treatment assigned)
    names: list
    late_true: float       # the mean effect of D on P(Y = 1) over the compliers of the sample
    types: np.ndarray      # (n,) int8: 0 complier, 1 always-taker, 2 never-taker

    @property
    def n(self):
        return self.X.shape[0]


def make_late_data(n: int = 50_000, seed: int = 1991, p_extra: int = 0, always_takers=True,
                   never_takers=True, params: DgpParams = TUTORIAL) -> LateData:
    """An encouragement design on the tutorial's covariates (``make_tutorial_data``): a
    mailing Z is assigned with a probability that depends on X, and the treatment taken D
    follows it only for the compliers. With s = sigmoid:

        Z ~ Bern(s(0.5 yob + 0.6 (g2002 - 0.8)))
        type: always-taker with probability s(-1.6 + 0.5 city), never-taker with probability
              s(-1.2 - 0.5 hh_size) (capped so the two sum to at most 1), else complier
        D = 1 for always-takers, 0 for never-takers, Z for compliers
        P(Y = 1) = 0.2 + 0.3 s(0.8 yob + 0.5 (g2000 - 0.85)) + tau D,
        tau = 0.2 + 0.1 sex for compliers, 0.05 for always-takers (never-takers: D = 0)

    so the effect differs by type and the LATE (the mean of tau over the compliers) is not
    the ATE. ``always_takers=False`` / ``never_takers=False`` drop that type: one-sided
    noncompliance. Every draw is a Philox function of (seed, stream, row)."""
    d = make_tutorial_data(n, seed, p_extra, params)
    X = d.X
    col = {k: X[:, j] for j, k in enumerate(d.names)}
    s = lambda v: 1.0 / (1.0 + np.exp(-v))
    idx = np.arange(n, dtype=np.uint64)
    Z = (_uniform(seed, S_Z, idx) < s(0.5 * col["yob"] + 0.6 * (col["g2002"] - 0.8))).astype(
        np.float64)
    p_at = s(-1.6 + 0.5 * col["city"]) if always_takers else np.zeros(n)
    p_nt = np.minimum(s(-1.2 - 0.5 * col["hh_size"]), 1.0 - p_at) if never_takers else np.zeros(n)
    u = _uniform(seed, S_TYPE, idx)
    types = np.where(u < p_at, 1, np.where(u >= 1.0 - p_nt, 2, 0)).astype(np.int8)
    D = np.where(types == 1, 1.0, np.where(types == 2, 0.0, Z))
    tau = np.where(types == 0, 0.2 + 0.1 * col["sex"], 0.05)
    base = 0.2 + 0.3 * s(0.8 * col["yob"] + 0.5 * (col["g2000"] - 0.85))
    Y = (_uniform(seed, S_YL, idx) < base + tau * D).astype(np.float64)
    return LateData(X=X, Y=Y, D=D, Z=Z, names=list(d.names), late_true=float(tau[types == 0].mean()),
                    types=types)


S_ARM = 73          # multi-arm data: the arm assigned
S_YM = 74           # multi-arm data: the outcome

ARM_NAMES = ("control", "civic_duty", "hawthorne", "self", "neighbors")
# the effect of each arm on P(Y = 1) at sex = 0.5: the control, then the four mailings in the
# experiment's order (its effects grow from civic duty to neighbours), then three stronger
# arms for designs with more than five levels
ARM_EFFECTS = (0.0, 0.018, 0.026, 0.049, 0.081, 0.10, 0.12, 0.14)


@dataclass
class MultiArmData:
    X: np.ndarray          # (n, p) float64, the tutorial's covariates
    Y: np.ndarray          # (n,) float64 in {0,1}
    D: np.ndarray          # (n,) float64 in {0, .., levels - 1}: the arm (0 = control)
    names: list
    arms: list             # the arms' names, by level
    apo_true: np.ndarray   # (levels,) the sample mean of P(Y = 1 | X, arm c), every row in arm c
    propensity: np.ndarray  # (n, levels) P(D = c | X)

    @property
    def n(self):
        return self.X.shape[0]


def make_multiarm_data(n: int = 50_000, seed: int = 1991, levels: int = 5, p_extra: int = 0,
                       params: DgpParams = TUTORIAL) -> MultiArmData:
    """The mailing experiment with all its arms on the tutorial's covariates
    (``make_tutorial_data``): a control group (level 0) and ``levels - 1`` mailings (2 <=
    levels <= 8; five is the experiment: civic duty, Hawthorne, self, neighbours), assigned
    with probabilities that depend on X, so the naive contrasts are biased. With s = sigmoid
    and u = 0.5 yob + 0.8 (g2000 - 0.85), yob the draw before standardisation:

        P(D = c | X) = softmax_c(a_c + b_c u),  a_0 = log(levels + 3), a_c = 0 (c >= 1),
                       b_c = 0.25 c  (the stronger the mailing, the more it goes to likely voters)
        P(Y = 1)     = 0.2 + 0.3 s(0.8 yob + 0.5 (g2000 - 0.85)) + tau_D,
        tau_c        = ARM_EFFECTS[c] (1 + 0.5 (sex - 0.5))

    ``apo_true[c]`` is the sample mean of P(Y = 1) had every row received arm c. Every draw is
    a Philox function of (seed, stream, row), and a row's D and Y are functions of (seed, row)
    alone (the standardised X depends on n through its column means)."""
    levels = int(levels)
    if not 2 <= levels <= len(ARM_EFFECTS):
        raise ValueError(f"levels must be in 2..{len(ARM_EFFECTS)}, got {levels}")
    d = make_tutorial_data(n, seed, p_extra, params)
    X = d.X
    col = {k: X[:, j] for j, k in enumerate(d.names)}
    s = lambda v: 1.0 / (1.0 + np.exp(-v))
    idx = np.arange(n, dtype=np.uint64)
    yob = _normal(seed, S_CTS + 0, idx)     # the unscaled draw: D and Y do not depend on n
    u = 0.5 * yob + 0.8 * (col["g2000"] - 0.85)
    score = np.stack([(np.log(levels + 3.0) if c == 0 else 0.0) + 0.25 * c * u
                      for c in range(levels)], axis=1)
    score -= score.max(axis=1, keepdims=True)
    prob = np.exp(score)
    prob /= prob.sum(axis=1, keepdims=True)
    cum = np.cumsum(prob, axis=1)
    cum[:, -1] = 1.0
    D = (_uniform(seed, S_ARM, idx)[:, None] >= cum).sum(axis=1).astype(np.float64)
    base = 0.2 + 0.3 * s(0.8 * yob + 0.5 * (col["g2000"] - 0.85))
    tau = np.asarray(ARM_EFFECTS[:levels])[None, :] * (1.0 + 0.5 * (col["sex"] - 0.5))[:, None]
    p_all = base[:, None] + tau
    Y = (_uniform(seed, S_YM, idx) < p_all[np.arange(n), D.astype(np.int64)]).astype(np.float64)
    arms = [ARM_NAMES[c] if c < len(ARM_NAMES) else f"arm{c}" for c in range(levels)]
    return MultiArmData(X=X, Y=Y, D=D, names=list(d.names), arms=arms,
                        apo_true=p_all.mean(axis=0), propensity=prob)


S_CL_U = 75         # clustered data: the cluster random effect
S_CL_E = 76         # clustered data: the row noise
S_CL_W = 77         # clustered data: the treatment (drawn per cluster or per row)

CLUSTER_TAU = 0.2   # the constant effect of make_clustered_data: PLR and IRM estimate the same


@dataclass
class ClusteredData:
    X: np.ndarray          # (n, p) float64, the tutorial's covariates
    Y: np.ndarray          # (n,) float64, continuous
    W: np.ndarray          # (n,) float64 in {0,1}
    clusters: np.ndarray   # (n,) int64 cluster label of every row
    names: list
    tau_true: float

    @property
    def n(self):
        return self.X.shape[0]


def make_clustered_data(n: int = 50_000, cluster_size: int = 5, icc: float = 0.3,
                        seed: int = 1991, assign: str = "cluster", p_extra: int = 0,
                        params: DgpParams = TUTORIAL) -> ClusteredData:
    """Rows that are dependent within clusters, on the tutorial's covariates
    (``make_tutorial_data``): row i belongs to cluster i // cluster_size, and with s = sigmoid

        Y = 0.5 yob + 0.3 g2000 + CLUSTER_TAU W + sqrt(icc) u_c + sqrt(1 - icc) e_i,
        u_c, e_i ~ N(0, 1): ``icc`` is the intra-cluster correlation of the noise
        assign="cluster": W_c ~ Bern(0.5), one draw per cluster (a cluster-randomised trial:
                          the i.i.d. SE is too small by about sqrt(1 + (m - 1) icc))
        assign="row":     W_i ~ Bern(s(0.5 yob)), one draw per row (the score's cluster sums
                          largely cancel: the two SEs are close)

    Every draw is a Philox function of (seed, stream, row or cluster)."""
    if assign not in ("cluster", "row"):
        raise ValueError(f'assign must be "cluster" or "row", got {assign!r}')
    if cluster_size < 1 or not 0.0 <= icc <= 1.0:
        raise ValueError("cluster_size must be >= 1 and icc in [0, 1]")
    d = make_tutorial_data(n, seed, p_extra, params)
    col = {k: d.X[:, j] for j, k in enumerate(d.names)}
    idx = np.arange(n, dtype=np.uint64)
    cl = (idx // np.uint64(cluster_size)).astype(np.int64)
    cid = cl.astype(np.uint64)
    if assign == "cluster":
        W = (_uniform(seed, S_CL_W, cid) < 0.5).astype(np.float64)
    else:
        W = (_uniform(seed, S_CL_W, idx) < 1.0 / (1.0 + np.exp(-0.5 * col["yob"]))).astype(
            np.float64)
    Y = 0.5 * col["yob"] + 0.3 * col["g2000"] + CLUSTER_TAU * W + \
        np.sqrt(icc) * _normal(seed, S_CL_U, cid) + np.sqrt(1.0 - icc) * _normal(seed, S_CL_E, idx)
    return ClusteredData(X=d.X, Y=Y, W=W, clusters=cl, names=list(d.names), tau_true=CLUSTER_TAU)


S_PL_Z = 80         # PLIV data: 80..83 the instruments' noise
S_PL_U = 84         # PLIV data: the unobserved confounder of D and Y
S_PL_D = 85         # PLIV data: the treatment's own noise
S_PL_Y = 86         # PLIV data: the outcome's noise

PLIV_THETA = 0.5    # the constant effect of make_pliv_data


@dataclass
class PlivData:
    X: np.ndarray          # (n, p) float64, the tutorial's covariates
    Y: np.ndarray          # (n,) float64, continuous
    D: np.ndarray          # (n,) float64, continuous: the endogenous treatment
    Z: np.ndarray          # (n, q) float64, continuous instruments
    names: list
    theta_true: float

    @property
    def n(self):
        return self.X.shape[0]


def make_pliv_data(n: int = 50_000, seed: int = 1991, q: int = 1, p_extra: int = 0,
                   strength: float = 0.5, params: DgpParams = TUTORIAL) -> PlivData:
    """A continuous treatment with an endogeneity problem on the tutorial's covariates
    (``make_tutorial_data``): a dose D driven by q instruments (1 <= q <= 4), by X and by a
    confounder U nobody observes, which also moves the outcome. With e ~ N(0, 1) draws,

        Z_j = 0.4 yob + 0.3 (g2000 - 0.85) (-1)^j + e_j                    j = 0..q-1
        D   = strength * sum_j Z_j / (1 + j) + 0.5 yob + 0.4 g2002 + U + 0.5 e_D
        Y   = PLIV_THETA D + 0.5 yob + 0.3 g2000 + U + e_Y

    The instruments depend on X (they are valid only after partialling X out) and reach Y
    through D alone; cov(D, U) > 0, so the partially linear regression of Y on D is biased
    upwards by about 1 / (strength^2 sum_j (1 + j)^-2 + 1.25), while PLIV recovers
    ``theta_true``. ``strength`` scales the first stage (0: irrelevant instruments). Every draw
    is a Philox function of (seed, stream, row)."""
    if not 1 <= q <= 4:
        raise ValueError(f"make_pliv_data draws 1 to 4 instruments, got q = {q}")
    d = make_tutorial_data(n, seed, p_extra, params)
    col = {k: d.X[:, j] for j, k in enumerate(d.names)}
    idx = np.arange(n, dtype=np.uint64)
    Z = np.column_stack([0.4 * col["yob"] + 0.3 * (col["g2000"] - 0.85) * (-1.0) ** j
                         + _normal(seed, S_PL_Z + j, idx) for j in range(q)])
    U = _normal(seed, S_PL_U, idx)
    D = strength * (Z / (1.0 + np.arange(q))).sum(1) + 0.5 * col["yob"] + 0.4 * col["g2002"] \
        + U + 0.5 * _normal(seed, S_PL_D, idx)
    Y = PLIV_THETA * D + 0.5 * col["yob"] + 0.3 * col["g2000"] + U + _normal(seed, S_PL_Y, idx)
    return PlivData(X=d.X, Y=Y, D=D, Z=Z, names=list(d.names), theta_true=PLIV_THETA)
