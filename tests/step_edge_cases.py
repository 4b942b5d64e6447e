"""The inputs of the step-edge tests, shared by tests/test_step_edges_cpu.py (the float64 reference against the oracle, the float32
restatement and its mutants against the bars) and tests/test_gpu_step_edges.py (the device against the reference): both must see
the same numbers, or the sensitivity check says nothing about the device test.  Plain numpy, seeded, no GPU.

A case is a dict as tests/step_ref.py describes it, with ``steps`` (one, or three chained through the running statistics),
``maxact0`` / ``phisum0_0`` (what the statistics hold before the first step), ``designed`` [N] (rows built to sit ON a branch: never
excluded), ``expect`` {row: {branch quantity: value}} (what the reference and the restatement must both say about a designed row of
the first step), ``nsubs`` (the lane counts it runs with on the device) and ``name``.

Unless a case says otherwise every input is chosen so that no float32 square or expf argument under- or overflows."""
import numpy as np

import step_ref as sr

F32 = np.float32
KMAX = 50
NS = (1, 3, 4, 5, 63, 64, 65, 257)      # a lone rollout, partial waves of 16-lane groups, a partial 256-block of k_modulate
KS = (0, 1, 15, 16, 17, KMAX)           # no kernel, one, fewer than the lanes, exactly the lanes, one wrap, n_kernel_max
KCLOSE = (1, 2, 5)
LIN_THR = F32(2.0 ** -6)
SENTINEL = np.array([0xFFFFFFFF], np.uint32).view(F32)[0]


def params(**over):
    """omds_params as float32 values: the reference's constants, with dst_thr, goal_act_cut and lin_thr dyadic so that the designed
    rows can hit them exactly."""
    p = dict(dt=0.5, dst_thr=0.25, lin_thr=LIN_THR, lvel=(0.0, 1.0, -1.0, 0.0, 10.0), ln=(0.0, 1.0, 0.0, 0.1, 100.0), ltau=(5.0, 1.0, 0.0, 0.1, 100.0),
             goal_act_cut=0.25, norm_clamp=0.5, coll_slow=0.1, coll_repulse=0.1, softmax_k=-10.0, rbf_p=2.0, variant=0)
    p.update(over)
    return {name: (tuple(F32(x) for x in v) if isinstance(v, tuple) else (int(v) if name == "variant" else F32(v))) for name, v in p.items()}


def to_params(prm):
    """The parameters of a case as the omds_params the hook takes."""
    from optimalmodulationds_amd import _lib
    p = _lib.default_params()
    for name, v in prm.items():
        if isinstance(v, tuple):
            for j, x in enumerate(v):
                getattr(p, name)[j] = float(x)
        else:
            setattr(p, name, int(v) if name == "variant" else float(v))
    return p


def random_case(name, n, N, K, k, seed, *, frame=False, H=2, step=1, A=None, seds=None, nsubs=None, O=6, **prm):
    """Random rows: gradients O(1), distances in [-0.2, 0.6] around dst_thr (ascending, as the top-k leaves them), states within
    2 rad of qf, kernel centres around the states.  qf is dyadic with qf[0] = 0: the designed rows write offsets that are exact."""
    rng = np.random.RandomState(seed)
    d = n + 3
    qf = (np.round(rng.uniform(-1, 1, n) * 4) / 4).astype(F32)
    qf[0] = 0
    dirs = rng.standard_normal((N, n))
    q = (qf + dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * rng.uniform(0.05, 2.0, (N, 1))).astype(F32)
    c = dict(name=name, n=n, k=k, d=d, K=K, Kmax=KMAX, H=H, qf=qf, prm=params(**prm), A=None if A is None else np.asarray(A, F32), seds=seds,
             gradx=rng.standard_normal((N, k, d)).astype(F32), drow=np.sort(rng.uniform(-0.2, 0.6, (N, k)), axis=1).astype(F32),
             frame=frame, frame_max=F32(1.0), vel=rng.uniform(-0.3, 0.3, (O, 3)).astype(F32), row_obs=rng.randint(0, O, (N, k)).astype(np.int32),
             steps=[dict(step=step, q=q, mu=(q[:, None, :] + 0.5 * rng.standard_normal((N, K, n))).astype(F32),
                         sigma=rng.uniform(0.5, 2.0, (N, K)).astype(F32), alpha=rng.standard_normal((N, K, n)).astype(F32))],
             maxact0=np.full((N, KMAX), SENTINEL, F32), phisum0_0=np.full(KMAX, SENTINEL, F32), designed=np.zeros(N, bool), expect={},
             nsubs=nsubs if nsubs is not None else ((1, 16) if n in (2, 7) and seds is None else (1,)))
    return c


def _along_goal(c, row):
    """Gradient rows of ``row`` along q - qf (so that g . vhat = -1 and 1 - l_vel is about 1) at a distance 0.03 above dst_thr
    (1 - l_n about 0.88): the activation is then ca va ga with ca va about 0.87, and a cut of ga shows in it."""
    x = c["steps"][0]["q"][row] - c["qf"]
    c["gradx"][row, :, :c["n"]] = x / max(float(np.abs(x).max()), 1e-30)
    c["drow"][row, :] = F32(0.28)


def shape_cases():
    out = []
    for i, N in enumerate(NS):
        for n in (2, 7):
            out.append(random_case(f"shape_N{N}_n{n}", n, N, KS[(i + n) % 6], KCLOSE[i % 3], 100 + 10 * i + n, frame=bool((i + n) % 2),
                                   rbf_p=(2.0, 1.0, 3.0)[i % 3], variant=i % 2))
    for i, K in enumerate(KS):
        for n in (2, 7):
            out.append(random_case(f"shape_K{K}_n{n}", n, 65, K, KCLOSE[(i + 1) % 3], 300 + 10 * i + n, frame=bool(i % 2), rbf_p=(2.0, 3.0, 1.0)[i % 3]))
    for n in (1, 3, 4, 5, 6):
        out.append(random_case(f"shape_n{n}", n, 65, KS[n % 6], KCLOSE[n % 3], 500 + n, frame=bool(n % 2), variant=n % 2))
        out.append(random_case(f"shape_n{n}_N257", n, 257, 17, 5, 520 + n, frame=not bool(n % 2)))
    return out


def lane_cases():
    """K = 0 and 1: the two lane counts perform the same operations in the same order (bit-identical outputs); K >= 2: only the order
    of the policy sum differs."""
    return [random_case(f"lanes_K{K}_n{n}_f{int(frame)}", n, 37, K, 5, 700 + 10 * K + n + int(frame), frame=frame)
            for K in (0, 1, 2, 17) for n in (2, 7) for frame in (False, True)]


def nominal_case(n):
    """Linear DS.  qf[0] = 0, so q[0] IS the offset: row 0 has q - qf = (lin_thr, 0, ..) with lin_thr = 2^-6: dst^2 = 2^-12 and its
    square root 2^-6 are exact, dst > lin_thr is false and v is not normalised.  Row 1 is one ulp above: x = 2^-6 (1 + 2^-23), x^2
    rounds to 2^-12 (1 + 2^-22), whose correctly rounded root is x again: normalised.  Row 2 is q == qf: v = 0, vhat = 0 / 0."""
    c = random_case(f"nominal_n{n}", n, 20, 3, 2, 800 + n)
    q = c["steps"][0]["q"]
    q[0:3] = c["qf"]
    q[0, 0] = LIN_THR
    q[1, 0] = np.nextafter(LIN_THR, F32(1))
    c["designed"][:3] = True
    c["expect"] = {0: dict(far=False), 1: dict(far=True)}
    return c


def matrix_cases(n):
    eye = np.eye(n, dtype=F32)
    sing = np.random.RandomState(810 + n).standard_normal((n, n)).astype(F32)
    sing[0] = 0                                    # row 0 zero: singular, and x = (1, 0, ..) gives v = 0 exactly, row 0 below
    c1 = random_case(f"matrix_minus_I_n{n}", n, 20, 3, 2, 820 + n, A=-eye)
    c2 = random_case(f"matrix_singular_n{n}", n, 20, 3, 2, 830 + n, A=sing)
    c2["steps"][0]["q"][0] = c2["qf"]
    c2["steps"][0]["q"][0, 0] = 1
    c2["designed"][0] = True
    return [c1, c2]


def blend_case(n):
    """Rows 0 / 1: two gradient rows with EQUAL distances and OPPOSITE gradients (k = 2: both weights are exactly 0.5 and the blended
    gradient exactly zero, g / |g| = 0 / 0), out of collision and in it.  Row 2: equal distances.  Row 3: distances 20 apart, the far
    row's weight expf(-200) underflows to 0.  Row 4: every distance 1e6, the all-links-ignored sentinel (softmax_k drow = -1e7: without
    the maximum subtracted every weight is 0 / 0)."""
    c = random_case(f"blend_n{n}", n, 20, 3, 2, 840 + n)
    for row, d0 in ((0, 0.375), (1, 0.125)):
        c["gradx"][row, 1] = -c["gradx"][row, 0]
        c["drow"][row] = F32(d0)
    c["drow"][2] = F32(0.3125)
    c["drow"][3] = (F32(0.3), F32(20.3))
    c["drow"][4] = F32(1e6)
    c["designed"][:5] = True
    c["expect"] = {0: dict(coll=False), 1: dict(coll=True)}
    return c


def blend_k5_case(n):
    c = random_case(f"blend_k5_n{n}", n, 20, 16, 5, 850 + n)
    c["drow"][0] = F32(0.3125)          # k equal distances
    c["drow"][1] = F32(1e6)
    c["drow"][2] = (F32(0.3), F32(0.3), F32(20.3), F32(20.3), F32(40.0))
    c["designed"][:3] = True
    return c


def collision_case(n):
    """Row 0: drow[0] == dst_thr, the difference is exactly 0: not in collision.  Row 1: one ulp below, the difference -2^-26 is
    exact: in collision.  Row 2: distance = -1 exactly (-0.75 - 0.25): expf(100 * 1.05) overflows inside gsig and the sigmoids are
    exactly their end values l_n = 0, l_tau = 5 (the NAMED overflow; float64 reaches them to 1e-45)."""
    c = random_case(f"collision_n{n}", n, 20, 3, 2, 860 + n)
    c["drow"][0] = (F32(0.25), F32(0.4))
    c["drow"][1] = (np.nextafter(F32(0.25), F32(0)), F32(0.4))
    c["drow"][2] = (F32(-0.75), F32(0.4))
    c["designed"][:3] = True
    c["expect"] = {0: dict(coll=False, distance=0.0), 1: dict(coll=True), 2: dict(coll=True, distance=-1.0)}
    return c


def goal_case(n):
    """goal_act_cut = 0.25, qf[0] = 0.  Row 0: q - qf = (0.25, 0, ..): sqrt(0.25) = 0.5 and 0.5^2 = 0.25 are exact, ga == cut stays on.
    Row 1: one ulp less, 0.25 - 2^-26: its root 0.5 sqrt(1 - 2^-24) lies just below the midpoint 0.5 - 2^-26 and rounds down to 0.5 - 2^-25,
    whose square rounds to 0.25 - 2^-25 < cut: cut to 0.  Row 2: far from the goal, ga clips at 1.  Row 3: q == qf, ga = 0.  The
    gradients of rows 0..2 point along q - qf close to the surface, so that ca va is about 0.87 and the cut shows in the activation."""
    c = random_case(f"goal_n{n}", n, 20, 3, 2, 870 + n)
    q = c["steps"][0]["q"]
    q[0:4] = c["qf"]
    q[0, 0] = F32(0.25)
    q[1, 0] = np.nextafter(F32(0.25), F32(0))
    q[2, 0] = F32(1.5)
    for row in (0, 1, 2):
        _along_goal(c, row)
    c["designed"][:4] = True
    c["expect"] = {0: dict(cut=False, ga_raw=0.25), 1: dict(cut=True), 2: dict(cut=False, ga_raw=1.0), 3: dict(cut=True, ga_raw=0.0)}
    return c


def clamp_case(n):
    """Sigmoids flat at 1 (y_min = y_max = 1: l_vel = l_n = l_tau = 1 exactly, so l_nv = 1, the activation 0 and u = v exactly) and
    A = -I (v = -x exactly).  Row 0: x = (0.5, 0, ..): |u| = sqrt(0.25) = 0.5 == norm_clamp exactly: NOT normalised.  Row 1: one ulp
    above: normalised.  Rows 2 / 3: |u| = 0.4995 / 0.5005, either side.  Row 4: sigmoids flat at 0 in a case of its own (below)."""
    flat = (1.0, 1.0, 0.0, 0.1, 100.0)
    c = random_case(f"clamp_n{n}", n, 20, 3, 2, 880 + n, A=-np.eye(n, dtype=F32), lvel=flat, ln=flat, ltau=flat)
    q = c["steps"][0]["q"]
    q[0:4] = c["qf"]
    q[0, 0], q[1, 0], q[2, 0], q[3, 0] = F32(0.5), np.nextafter(F32(0.5), F32(1)), F32(0.4995), F32(0.5005)
    c["designed"][:4] = True
    c["expect"] = {0: dict(clamped=True, unorm=0.5), 1: dict(clamped=False), 2: dict(clamped=True), 3: dict(clamped=False)}
    return c


def u_zero_case(n):
    """Sigmoids flat at 0: u = 0 vt + (0 gv) g = 0 on every row, |u| = 0 <= norm_clamp, u / 1 = 0: the step does not move."""
    flat = (0.0, 0.0, 0.0, 0.1, 100.0)
    c = random_case(f"u_zero_n{n}", n, 20, 3, 2, 890 + n, lvel=flat, ln=flat, ltau=flat)
    c["drow"] = np.abs(c["drow"]) + F32(0.3)          # out of collision
    c["designed"][:] = True
    c["expect"] = {0: dict(clamped=True, unorm=0.0)}
    return c


def policy_case(n, rbf_p, variant=0):
    """Row 0: mu == q for kernel 0: nrm = 0 (powf(0, p) for p != 2), phi = 1.  Row 1: sigma nrm^2 = 2000, phi = 0 (float64: 1e-869 = 0
    as well).  Row 2: a NaN alpha in kernel 1: the policy sum, vt and u are NaN, nan_to_num makes u = 0; no other rollout sees it."""
    c = random_case(f"policy_p{int(rbf_p)}_v{variant}_n{n}", n, 20, 17, 2, 900 + 10 * int(rbf_p) + n + variant, rbf_p=rbf_p, variant=variant)
    s = c["steps"][0]
    s["mu"][0, 0] = s["q"][0]
    s["mu"][1, 0] = s["q"][1]
    s["mu"][1, 0, 0] += F32(10.0)
    s["sigma"][1, 0] = F32(20.0)
    s["alpha"][2, 1, n - 1] = np.nan
    s["q"][2] = c["qf"] + F32(1.0)
    _along_goal(c, 2)                                   # the activation of row 2 is not 0: the NaN reaches u
    c["designed"][:3] = True
    return c


def sequence_case(n):
    """Steps 1, 2, 3 of H = 3 chained through maxact / phisum0, which hold garbage before step 1 (overwritten, not accumulated).  The
    states of steps 2 and 3 are fixed inputs (the float64 reference's own next states, rounded), so that every implementation sees the
    same ones.  sigma of kernel 1 of rollout 2 is NaN at step 2 only: maxact[2, 1] is NaN from step 2 on, nothing else is.  Step 3 ==
    H leaves the rollouts alone; steps 2 and 3 leave qdot alone."""
    c = random_case(f"sequence_n{n}", n, 20, 17, 2, 950 + n, H=3)
    rng = np.random.RandomState(960 + n)
    c["maxact0"] = rng.uniform(5, 9, c["maxact0"].shape).astype(F32)
    c["phisum0_0"] = rng.uniform(5, 9, KMAX).astype(F32)
    c["drow"] = (np.abs(c["drow"]) * F32(0.2) + F32(0.26)).astype(F32)     # near the surface, out of collision: the activations are not 0
    s1 = c["steps"][0]
    for i in (2, 3):
        prev = c["steps"][-1]
        o = sr.step(c, prev, c["maxact0"], c["phisum0_0"])
        nxt = dict(prev, step=i, q=(prev["q"].astype(np.float64) + o["dq"]).astype(F32), sigma=s1["sigma"].copy())
        if i == 2:
            nxt["sigma"][2, 1] = np.nan
        c["steps"].append(nxt)
    return c


def frame_cases(n):
    """k = 1 (w = 1 exactly), gradient rows (1, 0, .. | 1, 0, 0): |g| = 1 and rate = vel[.][0] exactly, frame_max = 1.  Rows 0 / 1: rate 2 and
    -2 clamp at +-1; row 2: 0.999 stays; row 3: an infinite velocity component, the rate is not finite and r = 0.  The second case has
    the exactly-zero blended gradient of blend_case under the frame: qo = 0."""
    c = random_case(f"frame_clamp_n{n}", n, 20, 3, 1, 970 + n, frame=True, O=20)
    c["row_obs"][:, 0] = np.arange(20)
    for row, v0 in ((0, 2.0), (1, -2.0), (2, 0.999), (3, np.inf)):
        c["gradx"][row, 0] = 0
        c["gradx"][row, 0, 0] = c["gradx"][row, 0, n] = 1
        c["vel"][row] = (v0, 0.125, -0.125)
    c["designed"][:4] = True
    z = blend_case(n)
    z.update(name=f"frame_zero_gradient_n{n}", frame=True)
    z["row_obs"][:2] = (0, 1)           # two spheres with different velocities: the rate is not 0, only |g| is
    return [c, z]


def seds_mixture(n, G, seed, lin_thr, seds_thr):
    """The test's own well-conditioned mixture: sigma_inv = Q diag(lambda) Q^T with lambda in [1, 10] (condition number <= 10),
    centres within 0.5 of the goal, A_j = -I + 0.3 noise, b_j = 0.3 noise, equal priors, den = sqrt((2 pi)^n / det sigma_inv)."""
    rng = np.random.RandomState(seed)
    mu_in = rng.standard_normal((G, n))
    mu_in = (mu_in / np.linalg.norm(mu_in, axis=1, keepdims=True) * rng.uniform(0, 0.5, (G, 1))).astype(F32)
    Si = np.zeros((G, n, n), F32)
    den = np.zeros(G, F32)
    for g in range(G):
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        lam = rng.uniform(1, 10, n)
        Si[g] = ((Q * lam) @ Q.T).astype(F32)
        den[g] = np.sqrt((2 * np.pi) ** n / np.prod(lam))
    return dict(mu_in=mu_in, b=(0.3 * rng.standard_normal((G, n))).astype(F32), sigma_inv=Si,
                A=(-np.eye(n) + 0.3 * rng.standard_normal((G, n, n))).astype(F32), prior=np.full(G, 1.0 / G, F32), den=den,
                lin_thr=float(F32(lin_thr)), seds_thr=float(F32(seds_thr)))


def seds_cases(n):
    """States within 1.5 of the goal (|x - mu| <= 2).  lin_thr = 0.5: rows inside are NEAR (v = y as it is); seds_thr = 0.01: the far
    rows are STRONG (v = y / |y|); seds_thr = 100 in the *_weak cases: the far rows are WEAK (the linear fallback -x / |x|).  Row 0: the
    state at the goal.  Row 1: x = (60, 0, ..), prob >= 3000 for every component: expf underflows (the NAMED underflow; float64's exp
    does too), psum == 0, pxi / psum = 0 / 0 -> 0, every beta is the 1e-8 floor."""
    out = []
    for G in (1, 2, 10, 64):
        for weak in (False, True):
            sd = seds_mixture(n, G, 1000 + 10 * G + n, 0.5, 100.0 if weak else 0.01)
            c = random_case(f"seds_G{G}_{'weak' if weak else 'strong'}_n{n}", n, 33, 3, 2, 1100 + 10 * G + n + int(weak), seds=sd)
            q, qf = c["steps"][0]["q"], c["qf"]
            x = q - qf
            q[:] = qf + x * np.minimum(1.0, 1.5 / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)
            q[0] = qf
            q[1] = qf
            q[1, 0] = F32(60.0)
            c["designed"][:2] = True
            c["expect"] = {0: dict(seds_far=False), 1: dict(seds_far=True, seds_weak=True)}
            out.append(c)
    return out


def all_cases():
    out = shape_cases() + lane_cases()
    for n in (2, 7):
        out += [nominal_case(n)] + matrix_cases(n) + [blend_case(n), blend_k5_case(n), collision_case(n), goal_case(n), clamp_case(n), u_zero_case(n)]
        out += [policy_case(n, 2.0), policy_case(n, 1.0), policy_case(n, 3.0), policy_case(n, 2.0, variant=1), sequence_case(n)]
        out += frame_cases(n) + seds_cases(n)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def at_rest(c):
    """The case with the frame on and every velocity zero: the device must return the bits of the case without the frame."""
    return dict(c, frame=True, vel=np.zeros_like(c["vel"]), name=c["name"] + "_at_rest")


# ---- the bars (the project's own, stage B of _check_teacher_forced) ---------------------------------------------------------------------
RTOL = 1e-5               # helpers.RTOL, relative to the largest reference magnitude of the output in the case
DIST_ATOL = 1e-6
# The one class that cannot meet RTOL of its own scale: the activation (and what is multiplied by it: maxact, and kval under
# KVAL_TIMES_ACT) in a case where EVERY rollout is far from the surface or moving away: act = (1 - l_n)(1 - l_vel) ga with l_n or
# l_vel within 1e-6 of 1, and float32 keeps 1 - l only to the rounding of l, whatever is left of it (shape_N1_n2: act = 1.3e-16 in
# float64, 0 in float32).  The class: cases whose largest activation is below ACT_ATOL / RTOL = 0.048.  Its bar is 4 x the
# restatement's worst error on the class, taken at the power of two above it: measured 8.9e-8 (printed by
# tests/test_step_edges_cpu.py, which holds the restatement to 2^-23 = 1.19e-7, one float32 spacing at 1), so 4 x 2^-23 absolute.
ACT_ATOL = 4 * 2.0 ** -23
VALUE_OUTPUTS = ("qdot", "dq", "normal", "dot", "act", "kval", "maxact", "phisum0")


def reference_outputs(c, o, q=None):
    """The outputs of one step as the device returns them, from a step_ref result (any dtype) -> dict of float64 arrays, None where the
    step leaves the buffer alone.  With ``q`` (the float32 restatement): q_next - q as it is recovered from the device's q_next."""
    K = c["K"]
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    dq = None if o["q_next"] is None else (f(o["dq"]) if q is None else f(o["q_next"]) - f(q))
    return dict(qdot=f(o["qdot"]), dq=dq, normal=f(o["normal"]), dot=f(o["dot"]), act=f(o["act"]),
                kval=f(o["kval"]), maxact=f(o["maxact"][:, :K]), phisum0=f(o["phisum0"][:K]), dist=f(o["dist"]))


def compare(c, ref, got, keep):
    """Errors of ``got`` against ``ref`` (both from reference_outputs) over the rows ``keep``: -> {output: error / bar}, the non-finite
    patterns compared exactly (a mismatch is reported as inf).  phisum0 belongs to rollout 0 and is compared whatever ``keep`` says."""
    res = {}
    for name in VALUE_OUTPUTS + ("dist",):
        r, g = ref[name], got[name]
        if r is None or g is None:
            res[name] = 0.0 if (r is None) == (g is None) else np.inf
            continue
        if name != "phisum0":
            r, g = r[keep], g[keep]
        if r.size == 0:
            res[name] = 0.0
            continue
        if not (np.array_equal(np.isnan(r), np.isnan(g)) and np.array_equal(np.isposinf(r), np.isposinf(g)) and np.array_equal(np.isneginf(r), np.isneginf(g))):
            res[name] = np.inf
            continue
        fin = np.isfinite(r)
        err = float(np.abs(r[fin] - g[fin]).max()) if fin.any() else 0.0
        scale = float(np.abs(r[fin]).max()) if fin.any() else 0.0
        bar = DIST_ATOL if name == "dist" else RTOL * scale
        if name in ("act", "maxact") or (name == "kval" and int(c["prm"]["variant"]) & sr.KVAL_TIMES_ACT):
            bar = max(bar, ACT_ATOL)
        res[name] = 0.0 if err == 0.0 else (err / bar if bar > 0 else np.inf)
    return res


def kept_rows(c, ref_step):
    """[N] bool: the rows of a step that are compared: every designed row, and the random rows whose float64 branch quantities stay
    clear of their thresholds (step_ref.near_threshold)."""
    return c["designed"] | ~sr.near_threshold(c, ref_step)


def errors(c, refs, gots):
    """Worst error / bar per output over the steps of a case: ``refs`` the float64 step_ref results, ``gots`` one reference_outputs
    dict per step."""
    worst = {}
    for s, o, got in zip(c["steps"], refs, gots):
        for name, e in compare(c, reference_outputs(c, o), got, kept_rows(c, o)).items():
            worst[name] = max(worst.get(name, 0.0), e)
    return worst


def expectations_met(c, o):
    """The branch outcomes a case states for its designed rows (first step), on a step_ref result of any dtype -> list of misses."""
    return [(row, key, want, o[key][row]) for row, exp in c["expect"].items() for key, want in exp.items() if not o[key][row] == want]
