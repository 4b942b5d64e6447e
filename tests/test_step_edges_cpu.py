"""tests/step_ref.py and tests/step_edge_cases.py on the CPU, so that tests/test_gpu_step_edges.py can lean on them:

1. the float64 reference against independent code: oracle.modulation_step on the golden scenario fixtures (fed the oracle's own
   distance_repulsion_nn outputs), oracle.seds_velocity and the reference's own answers on the SEDS fixtures, and frame_step /
   frame_quantities of tests/test_moving_frame_cpu.py;
2. the float32 restatement (step_ref.step(T=float32): the device's order of operations) meets the bars against the reference on
   ALL cases -- the bars are attainable in float32 on exactly these inputs -- with the same non-finite patterns and the branch
   outcomes the designed rows state;
3. the cases have teeth: every mutant of step_ref.MUTANTS misses a bar or an exact assertion on at least one case;
4. the random rows excluded for sitting within 1e-6 of a branch threshold are at most 1 % of any case's random rows."""
import numpy as np
import pytest

import step_edge_cases as sec
import step_ref as sr
from helpers import RTOL, SCENARIOS, SEDS_FILES, assert_close, load, seds_of, weights_path
from oracle import omds_oracle as orc

F32 = np.float32
_CACHE = {}


def cases():
    if not _CACHE:
        _CACHE["cases"] = sec.all_cases()
        _CACHE["refs"] = {c["name"]: sr.run(c) for c in _CACHE["cases"]}
    return _CACHE["cases"], _CACHE["refs"]


def _one_step_case(q, qf, drow, gradx, mu, sg, al, prm, *, A=None, seds=None, frame=False, vel=None, row_obs=None, frame_max=1.0, variant=0):
    N, n = q.shape
    K = sg.shape[1]
    c = dict(n=n, k=drow.shape[1], d=gradx.shape[2], K=K, Kmax=max(K, 1), H=2, qf=np.asarray(qf, F32), A=A, seds=seds, frame=frame, vel=vel,
             row_obs=row_obs, frame_max=frame_max, gradx=np.asarray(gradx, F32), drow=np.asarray(drow, F32),
             prm=sec.params(dst_thr=prm.dst_thr, lin_thr=prm.lin_thr, rbf_p=float(prm.p), variant=variant, goal_act_cut=prm.goal_act_cut,
                            norm_clamp=prm.norm_clamp, softmax_k=prm.softmax_k, lvel=prm.lvel, ln=prm.ln, ltau=prm.ltau))
    s = dict(step=1, q=np.asarray(q, F32), mu=mu, sigma=sg, alpha=al)
    return c, s, sr.step(c, s, np.zeros((N, max(K, 1))), np.zeros(max(K, 1)))


# ---- 1. the reference against independent code ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s for s in SCENARIOS if "seds" not in s])     # the SEDS branch: the SEDS fixtures below
def test_reference_against_the_oracle_step(name):
    fx = load(name)
    m = orc.Mlp.from_npz(weights_path(str(fx["kind"])))
    prm = orc.Params(dst_thr=float(fx["dst_thr"]), lin_thr=float(fx["lin_thr"]), p=int(fx["p"]), seds=seds_of(fx))
    q = np.ascontiguousarray(fx["it0_all_traj"][:, 0, :])
    mu, sg, al = fx["it0_mu_tmp"], fx["it0_sigma_tmp"], fx["it0_alpha_tmp"]
    d_orc, g_orc, _, _ = orc.distance_repulsion_nn(m, q, fx["obs"], int(fx["k"]), fx["ignored_links"])
    st = orc.modulation_step(q, fx["qf"], d_orc, g_orc, mu, sg, al, prm)
    # the blended gradient as ONE gradient row (weight 1): the blend itself is pinned by the moving-frame restatement below
    c, s, o = _one_step_case(q, fx["qf"], d_orc[:, None], g_orc[:, None, :], mu, sg, al, prm, seds=seds_of(fx))
    keep = ~sr.near_threshold(c, o)
    assert keep.mean() > 0.9
    assert_close(o["dist"][keep], st["distance"][keep], 1e-6, "distance")
    for mine, theirs in (("normal", "ghat"), ("dot", "dot"), ("act", "act"), ("phi", "phi"), ("u", "u")):
        assert_close(o[mine][keep], st[theirs][keep], RTOL, mine, floor=0.0 if mine == "u" else 1.0)


@pytest.mark.parametrize("name", SEDS_FILES)
def test_reference_against_the_seds_fixtures(name):
    """SEDS.get_velocity on the reference's shipped mixtures, at the 5e-5 of the largest output that
    tests/test_oracle_golden.py::test_seds_velocity grants the oracle.  Far from every component these states live on float32's
    RANGE (expf underflows, the responsibilities become the 1e-8 floor): the float64 reference models that (step_ref.f32_range) and
    then meets the reference's own answers on EVERY state of the three 7-D mixtures.  seds_2d is fitted in pixel units (condition
    number 1e8; b + A (x - mu) cancels three digits near its goal): there float32 itself is only good to a few 1e-4, so it is the
    float32 mode of the same code that is held to the reference's answers, and the float64 mode to 1e-3."""
    fx = load(name)
    sd = dict(mu_in=fx["mu_in"], b=fx["b"], sigma_inv=fx["sigma_inv"], A=fx["A"], prior=fx["prior"], den=fx["den"], lin_thr=float(fx["lin_thr"]),
              seds_thr=float(fx["seds_thr"]))
    x = fx["x"].astype(F32) - fx["xT"].reshape(1, -1).astype(F32)
    with np.errstate(all="ignore"):
        v64, dst, yn, _, _ = sr.seds_nominal(x.astype(np.float64), sd, np.float64)
        v32 = sr.seds_nominal(x, sd, F32)[0]
        y_orc = orc.seds_velocity(fx["x"], fx["xT"].reshape(-1), **sd)
    clear = (np.abs(dst - float(F32(sd["lin_thr"]))) > 1e-6) & (np.abs(yn - float(F32(sd["seds_thr"]))) > 1e-6)
    assert clear.mean() > 0.95
    e32 = assert_close(v32[clear], fx["y"][clear], 5e-5, "float32 mode vs the reference's")
    assert_close(v32[clear], y_orc[clear], 5e-5, "float32 mode vs the oracle's")
    e64 = assert_close(v64[clear], fx["y"][clear], 1e-3 if name == "seds_2d" else 5e-5, "float64 mode vs the reference's")
    print(f"{name}: against the reference's own answers: float32 mode {e32:.2e}, float64 mode {e64:.2e}")


def test_reference_against_the_moving_frame_restatement():
    import test_moving_frame_cpu as mf
    fc = mf.franka_case("emit")
    q = np.tile(fc["q_cur"], (fc["N"], 1)).astype(F32)
    q += (0.05 * np.random.RandomState(2).standard_normal(q.shape)).astype(F32)
    mu, sg, al = fc["samples"]
    n, k = q.shape[1], fc["k"]
    grad, d, w, sort_idx = mf.network_rows(fc["m"], q, fc["obs"], k, fc["ignored"], fc["prm"].softmax_k)
    fs = mf.frame_step(fc["m"], q, fc["qf"], fc["obs"], fc["vel"], k, fc["ignored"], mu, sg, al, fc["prm"], 0.25)
    rate, qo, g_raw, _ = mf.frame_quantities(grad, d, w, sort_idx, fc["vel"], n, 0.25)
    c, s, o = _one_step_case(q, fc["qf"], d, grad.reshape(q.shape[0], k, -1), mu, sg, al, fc["prm"], frame=True, vel=fc["vel"], row_obs=sort_idx,
                             frame_max=0.25)
    keep = ~sr.near_threshold(c, o)
    assert keep.mean() > 0.9 and (np.abs(o["ratio"]) > 0.25).any() and (np.abs(o["ratio"]) < 0.25).any(), "the clamp acts on some rows only"
    assert_close(o["rate"], rate, RTOL, "rate", floor=float(np.abs(rate).max()))
    assert_close(o["qo"][keep], qo[keep], RTOL, "qo", floor=0.0)
    assert_close(o["dist"][keep], fs["distance"][keep], 1e-6, "distance")
    for mine, theirs in (("normal", "ghat"), ("dot", "dot"), ("act", "act"), ("kval", "kval"), ("u", "u")):
        assert_close(o[mine][keep], fs[theirs][keep], RTOL, mine, floor=0.0 if mine == "u" else 1.0)


# ---- 2. the bars are attainable in float32 on these inputs -------------------------------------------------------------------------------
def _restated(c, mutant=None):
    outs = sr.run(c, F32, mutant)
    return outs, [sec.reference_outputs(c, o, s["q"]) for s, o in zip(c["steps"], outs)]


def test_float32_restatement_meets_the_bars_on_every_case():
    cs, refs = cases()
    worst, act_abs = {}, (0.0, "")
    for c in cs:
        outs, gots = _restated(c)
        e = sec.errors(c, refs[c["name"]], gots)
        for o64, got in zip(refs[c["name"]], gots):      # the class of sec.ACT_ATOL: activations below 0.048 everywhere in the case
            r = sec.reference_outputs(c, o64)
            if np.nanmax(np.abs(r["act"])) * sec.RTOL < sec.ACT_ATOL:
                err = float(np.nanmax(np.abs(r["act"] - got["act"])))
                act_abs = max(act_abs, (err, c["name"]))
        for name, v in e.items():
            if v > worst.get(name, (0.0, ""))[0]:
                worst[name] = (v, c["name"])
        assert max(e.values()) <= 1.0, f"{c['name']}: error / bar {e}"
        for o in (refs[c["name"]][0], outs[0]):
            assert not sec.expectations_met(c, o), (c["name"], sec.expectations_met(c, o))
        for o64, o32 in zip(refs[c["name"]], outs):      # what a step leaves alone
            assert (o64["q_next"] is None) == (o32["q_next"] is None) and (o64["qdot"] is None) == (o32["qdot"] is None)
    print("float32 restatement against the float64 reference, worst error / bar per output (bar: 1e-5 of the output's largest magnitude"
          " in the case; dist: 1e-6):")
    for name, (v, where) in sorted(worst.items()):
        print(f"  {name:8s} {v:.3f}  ({where})")
    print(f"cases whose activations are all below {sec.ACT_ATOL / sec.RTOL:.3f}: worst absolute error of the activation {act_abs[0]:.3e} ({act_abs[1]}); "
          f"their bar is 4 x 2^-23 = {sec.ACT_ATOL:.3e}")
    assert act_abs[0] <= 2.0 ** -23


def test_designed_rows_say_what_they_were_built_for():
    """The non-finite outcomes the reference states: q == qf gives u = 0, q_next = q and dot = NaN; the exactly-zero blended gradient
    gives a NaN normal and, in collision, a NaN next state; a NaN alpha is swallowed by nan_to_num; a NaN sigma sticks to maxact."""
    cs, refs = cases()
    by = {c["name"]: (c, refs[c["name"]]) for c in cs}
    for n in (2, 7):
        c, (o,) = by[f"nominal_n{n}"]
        assert not o["u"][2].any() and np.array_equal(o["q_next"][2], c["steps"][0]["q"][2]) and np.isnan(o["dot"][2]) and np.isnan(o["act"][2])
        c, (o,) = by[f"blend_n{n}"]
        assert np.isnan(o["normal"][:2]).all() and not o["u"][0].any() and np.isnan(o["q_next"][1]).all() and np.isfinite(o["q_next"][2:]).all()
        c, (o,) = by[f"frame_zero_gradient_n{n}"]
        assert not o["qo"][:2].any() and o["rate"][0] != 0
        c, (o,) = by[f"frame_clamp_n{n}"]
        assert np.allclose(np.linalg.norm(o["qo"][:4], axis=1), [1, 1, 0.999, 0]) and not np.isfinite(o["rate"][3])
        c, (o,) = by[f"policy_p2_v0_n{n}"]
        assert o["phi"][0, 0] == 1 and o["phi"][1, 0] == 0 and not o["u"][2].any() and o["act"][2] > 0.5 and np.isfinite(o["u"]).all()
        c, (o1, o2, o3) = by[f"sequence_n{n}"]
        for o, nan_now in ((o1, False), (o2, True), (o3, True)):
            m = np.isnan(o["maxact"][:, :c["K"]])
            assert m[2, 1] == nan_now and m.sum() == int(nan_now)
        assert np.allclose(o3["phisum0"][:c["K"]], o1["phi"][0] + o2["phi"][0] + o3["phi"][0]) and o3["q_next"] is None and o2["qdot"] is None
        for G in (1, 2, 10, 64):
            c, (o,) = by[f"seds_G{G}_strong_n{n}"]
            assert o["seds_far"].sum() > 5 and (~o["seds_far"]).sum() > 3 and not o["seds_weak"][o["seds_far"]][1:].all()
            assert np.allclose(o["v"][1], [-1] + [0] * (n - 1), atol=1e-12) and o["seds_yn"][1] < 1e-4, "psum == 0: every beta the floor, the linear fallback"


# ---- 3. the cases have teeth ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_every_mutant_is_caught(mutant):
    cs, refs = cases()
    for c in sorted(cs, key=lambda c: c["name"].startswith(("shape", "lanes", "seds"))):      # the designed cases first
        outs, gots = _restated(c, mutant)
        e = sec.errors(c, refs[c["name"]], gots)
        missed = sec.expectations_met(c, outs[0])
        if max(e.values()) > 1.0 or missed:
            over = {name: round(v, 1) for name, v in e.items() if v > 1.0}
            print(f"mutant {mutant}: caught by case {c['name']} (error / bar {over}, branch outcomes missed {missed})")
            return
    pytest.fail(f"no case catches the mutant {mutant}")


# ---- 4. the exclusions stay small -----------------------------------------------------------------------------------------------------------
def test_excluded_rows_are_at_most_one_percent_of_any_case():
    cs, refs = cases()
    total = rows = 0
    largest = 0.0
    for c in cs:
        for o in refs[c["name"]]:
            random_rows = ~c["designed"]
            out = random_rows & ~sec.kept_rows(c, o)
            total, rows = total + int(out.sum()), rows + int(random_rows.sum())
            if random_rows.any():
                share = out.sum() / random_rows.sum()
                if share > 0:
                    print(f"{c['name']}: {int(out.sum())} of {int(random_rows.sum())} random rows excluded ({100 * share:.2f} %)")
                largest = max(largest, float(share))
                assert share <= 0.01, (c["name"], share)
    print(f"excluded in all: {total} of {rows} random rows; the largest share of any case: {100 * largest:.2f} %")


# ---- 5. the hook refuses what it cannot run: a status code, before anything is launched (so this runs without a GPU) ------------------------
def test_hook_refuses_bad_arguments():
    import __graft_entry__ as g
    g.build()
    from optimalmodulationds_amd import _lib
    to_params = sec.to_params

    def call(c, **over):
        s = c["steps"][0]
        kw = dict(nsub=1, step=1, H=c["H"], prm=to_params(c["prm"]), qf=c["qf"], q=s["q"], drow=c["drow"], gradx=c["gradx"], mu=s["mu"], sigma=s["sigma"],
                  alpha=s["alpha"], Kmax=c["Kmax"], A=c["A"], seds=c["seds"], frame=c["frame"], frame_max=float(c["frame_max"]), vel=c["vel"],
                  row_obs=c["row_obs"], check=False)
        kw.update(over)
        return _lib.modulate_step(**kw)

    c7, c3 = sec.random_case("a", 7, 5, 3, 2, 1, frame=True), sec.random_case("b", 3, 5, 3, 2, 2)
    seds = sec.random_case("c", 7, 5, 3, 2, 3, seds=sec.seds_mixture(7, 2, 1, 0.5, 0.01))
    low, high = c7["row_obs"].copy(), c7["row_obs"].copy()
    low[4, 1], high[0, 0] = -1, c7["vel"].shape[0]
    big = sec.seds_mixture(7, 65, 1, 0.5, 0.01)
    bad_p = to_params(c7["prm"])
    bad_p.rbf_p = 0.0
    refused = [call(c7, nsub=2), call(c7, nsub=0), call(c3, nsub=16), call(seds, nsub=16), call(c7, step=0), call(c7, step=3), call(c7, H=0, step=0),
               call(c7, Kmax=2), call(c7, row_obs=low), call(c7, row_obs=high), call(c7, frame_max=float("nan")), call(c7, frame_max=-1.0),
               call(c7, gradx=c7["gradx"][:, :, :6]), call(c7, vel=c7["vel"][:, :2]), call(c7, gradx=np.tile(c7["gradx"], (1, 17, 1)), drow=np.tile(c7["drow"], (1, 17)),
                                                                                             row_obs=np.tile(c7["row_obs"], (1, 17))),
               call(seds, seds=big), call(seds, A=np.eye(7, dtype=F32)), call(c7, prm=bad_p), call(c7, H=65)]
    assert refused == [1] * len(refused), refused
