"""Cases of the schedule pin (tests/test_gpu_schedule_pin.py) and of its maker (tests/golden/make_schedule_pin.py): small fixtures
with large fronts, several steps and (lns_3937) one rank-deficient reschedule, factorized twice on one plan under every setting
that makes the planner or the step scheduler take another path.  What is kept per factorization is exact: launch and step
counts, the device memory held, rank and rh_total, and SHA-256 digests of the factors."""
import hashlib
import os

import numpy as np

from stmmqr_testlib import Symbolic, load_golden, scalar

FIXTURES = ("syn_grid3d", "grid20_standin", "epb1", "lns_3937")
STATS = ("nlaunch", "nsteps", "nlevels", "npanel_launch", "nupdate_launch", "retries", "reschedules", "device_bytes")
DIGESTS = ("HTau", "HStair", "Rdead", "Rblock_off")          # ... and Stack[:rh_total]

# name -> (options, environment)
SETTINGS = {
    "defaults": ({}, {}),
    "lookahead1_la_min0": (dict(lookahead=1), {"STMMQR_LA_MIN": "0"}),
    "lookahead0": (dict(lookahead=0), {}),
    "fused_update": (dict(fused_update=1), {}),
    "no_passengers": ({}, {"STMMQR_PASSENGERS": "0"}),
    "no_ca_riders": ({}, {"STMMQR_CA_RIDERS": "0"}),
    "pass_maxwg1": ({}, {"STMMQR_PASS_MAXWG": "1"}),
    "no_early_end": ({}, {"STMMQR_EARLY_END": "0"}),
    "recycle2": ({}, {"STMMQR_RECYCLE": "2"}),
    "recycle0": ({}, {"STMMQR_RECYCLE": "0"}),
    "pair1": (dict(big_front_cols=16, pair_update=1), {"STMMQR_PAIR_MIN": "1"}),
    "pair4": (dict(big_front_cols=16, pair_update=4), {"STMMQR_PAIR_MIN": "1"}),
    "panel_algo1": (dict(big_front_cols=16, panel_algo=1), {}),
    "panel_algo2": (dict(big_front_cols=16, panel_algo=2), {}),
    "graph": (dict(use_graph=1), {}),                        # default look-ahead: one stream, no parallel branches in the graph
}
CASES = [(f, s) for f in FIXTURES for s in SETTINGS]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record(st, N):
    out = {k: int(st[k]) for k in STATS}
    out["rank"], out["rh_total"] = int(N.rank), int(N.rh_total)
    out["Stack"] = sha(N.Stack[:N.rh_total])
    for k in DIGESTS:
        out[k] = sha(getattr(N, k))
    return out


def run_case(pkg, fixture, setting):
    """[record after the first factorization, record after the second one of the same plan]; options and environment restored."""
    g = load_golden(fixture)
    S = Symbolic(g)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}}
    tol, ntol = scalar(g, "in_tol"), int(scalar(g, "in_ntol"))
    opts, env = SETTINGS[setting]
    saved_opts = pkg.get_options()
    saved_env = {k: os.environ.get(k) for k in env}
    out = []
    try:
        pkg.set_options(**opts)
        os.environ.update(env)
        plan = pkg.HipQR(sym)
        try:
            st = plan.factorize(g["in_Ax"], tol, ntol, g["in_Ap"], g["in_Ai"])
            out.append(record(st, plan.download()))
            st = plan.factorize(g["in_Ax"], tol, ntol)
            out.append(record(st, plan.download()))
        finally:
            plan.close()
    finally:
        for k, v in saved_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        pkg.set_options(**saved_opts)
    return out
