"""One horizon step behind the distance network (csrc/step_device.h: modulate_core) in plain numpy, operation by operation in the
order of the device code: the nominal DS (linear, matrix, SEDS), the softmax blend of the k gradient rows, the moving frame
(include/omds.h: THE MOVING FRAME), the three sigmoids and the activations, the RBF policy with its running statistics, the
closed-form M v, the norm clamp, nan_to_num, the collision fix-up and the Euler step.

``step(c, s, maxact, phisum0)`` is the float64 REFERENCE of tests/test_gpu_step_edges.py.  ``step(..., T=np.float32)`` is the same
sequence of operations with every one of them rounded to float32 (numpy rounds products and sums separately; the device fuses the
multiply-adds the source writes in one expression, which is inside the bars): the RESTATEMENT tests/test_step_edges_cpu.py holds
against the reference, to show that the bars can be met in float32 on exactly the inputs of tests/step_edge_cases.py.  ``mutant``
names one deliberate mistake of MUTANTS; the CPU test shows that the cases catch each.

Where the device's result depends on the RANGE of float32 and not on its rounding, the reference models it: nan_to_num maps what
exceeds FLT_MAX in magnitude to +-FLT_MAX and NaN to 0, the approach rate of the moving frame counts as non-finite beyond
FLT_MAX, and the responsibilities of SEDS underflow where expf does (f32_range).  The parameters are the float32 values the device receives (``c["prm"]`` holds them as numpy float32).

A case ``c``: n, k, d, K, Kmax, H, qf [n], prm (dict), gradx [N, k, d], drow [N, k], A [n, n] or None, seds (dict of the arrays
omds_set_ds_seds takes) or None, frame (bool), frame_max, vel [O, ldVel], row_obs [N, k].  A step ``s``: step (1..H), q [N, n], mu
[N, K, n], sigma [N, K], alpha [N, K, n].  All inputs float32."""
import warnings

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
KVAL_TIMES_ACT = 1      # OMDS_VARIANT_KVAL_TIMES_ACT

MUTANTS = ("clamp_lt", "coll_le", "lin_ge", "cut_le", "no_nan_to_num", "maxact_fmax", "phisum0_no_reset", "softmax_no_max", "no_rate_clamp",
           "repulse_v", "policy_first16")


def nan_to_num(x):
    """torch.nan_to_num at float32's range, in the dtype of x."""
    T = x.dtype.type
    x = np.where(x != x, T(0), x)
    return np.where(x > T(FLT_MAX), T(FLT_MAX), np.where(x < T(-FLT_MAX), T(-FLT_MAX), x))


def f32_range(x):
    """A float64 array with float32's RANGE: magnitudes below the smallest normal float32 are rounded onto the subnormal grid (0
    below half the smallest subnormal), those beyond FLT_MAX become infinite; everything else keeps its float64 value.  (A float32
    array is returned as it is.)  The responsibilities of SEDS need it: far from every component expf underflows, the sum is 0 and
    every beta becomes the floor, where float64's exp would still tell the components apart."""
    if x.dtype == np.float32:
        return x
    tiny = np.abs(x) < float(np.finfo(np.float32).tiny)
    return np.where(tiny | (np.abs(x) > FLT_MAX), x.astype(np.float32).astype(np.float64), x)


def _gsig(x, s, T):
    c = (T(s[2]) + T(s[3])) * T(0.5)
    return T(s[0]) + (T(s[1]) - T(s[0])) / (T(1) + np.exp(T(s[4]) * (-x + c)))


def _sumsq(x, T):
    acc = np.zeros(x.shape[0], T)
    for j in range(x.shape[1]):
        acc = acc + x[:, j] * x[:, j]
    return acc


def _dotrows(a, b, T):
    acc = np.zeros(a.shape[0], T)
    for j in range(a.shape[1]):
        acc = acc + a[:, j] * b[:, j]
    return acc


def seds_nominal(x, sd, T):
    """SEDS.get_velocity on x = q - q_goal [N, n] (SEDS.py:34-74) -> (v, dst, yn)."""
    N, n = x.shape
    mu_in, b, Si, A = (np.asarray(sd[name]).astype(T) for name in ("mu_in", "b", "sigma_inv", "A"))
    prior, den = np.asarray(sd["prior"]).astype(T), np.asarray(sd["den"]).astype(T)
    G = prior.shape[0]
    dst2 = _sumsq(x, T)
    pxi = np.zeros((N, G), T)
    for g in range(G):
        dd = x - mu_in[g][None]
        prob = np.zeros(N, T)
        for cc in range(n):
            t = np.zeros(N, T)
            for r in range(n):
                t = t + dd[:, r] * Si[g, r, cc]
            prob = prob + t * dd[:, cc]
        pxi[:, g] = f32_range(prior[g] * f32_range(f32_range(np.exp(T(-0.5) * prob)) / den[g]))
    psum = np.zeros(N, T)
    for g in range(G):
        psum = psum + pxi[:, g]
    ysum = np.zeros((N, n), T)
    floor = T(np.float32(1e-8))
    for g in range(G):
        dd = x - mu_in[g][None]
        beta = nan_to_num(pxi[:, g] / psum)
        beta = np.where(beta < floor, floor, beta)
        for r in range(n):
            yj = np.full(N, b[g, r], T)
            for cc in range(n):
                yj = yj + A[g, r, cc] * dd[:, cc]
            ysum[:, r] = ysum[:, r] + beta * yj
    dst, yn = np.sqrt(dst2), np.sqrt(_sumsq(ysum, T))
    far, weak = dst > T(np.float32(sd["lin_thr"])), yn < T(np.float32(sd["seds_thr"]))
    v = np.where(far[:, None], np.where(weak[:, None], -x / dst[:, None], ysum / yn[:, None]), ysum)
    return v, dst, yn, far, weak


def step(c, s, maxact, phisum0, T=np.float64, mutant=None):
    """-> dict: u [N, n] (qdot), dq = dt u, q_next = q + dq (None at step == H: trajT is left alone), qdot (None behind step 1),
    dist, dot, act [N], normal [N, n], kval [N, K], phi [N, K], maxact [N, Kmax] and phisum0 [Kmax] (entries from K on are the ones
    given), v (the nominal velocity), and the branch quantities: distance, coll, ga_raw, cut, unorm, clamped, dst, far (linear DS), seds_dst, seds_yn, seds_far,
    seds_weak (SEDS), ratio = rate / |g| (frame)."""
    assert mutant is None or mutant in MUTANTS
    P, n, k, d, K, i = c["prm"], c["n"], c["k"], c["d"], c["K"], s["step"]
    q, qf = s["q"].astype(T), c["qf"].astype(T)
    N = q.shape[0]
    out = {}
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        x = q - qf[None]
        # nominal DS
        if c.get("seds") is not None:
            v, out["seds_dst"], out["seds_yn"], out["seds_far"], out["seds_weak"] = seds_nominal(x, c["seds"], T)
        elif c.get("A") is None:
            dst = np.sqrt(_sumsq(x, T))
            far = (dst >= T(P["lin_thr"])) if mutant == "lin_ge" else (dst > T(P["lin_thr"]))
            v = np.where(far[:, None], -x / dst[:, None], -x)
            out["dst"], out["far"] = dst, far
        else:
            A = np.asarray(c["A"]).astype(T)
            v = np.zeros((N, n), T)
            for j in range(n):
                for r in range(n):
                    v[:, j] = v[:, j] + x[:, r] * A[r, j]
        out["v"] = v
        vnorm = np.sqrt(_sumsq(v, T))
        vhat = v / vnorm[:, None]
        # softmax blend of the k gradient rows
        dr, gx = c["drow"].astype(T), c["gradx"].astype(T)
        a = T(P["softmax_k"]) * dr
        mx = np.zeros(N, T) if mutant == "softmax_no_max" else np.max(a, axis=1)
        e = np.exp(a - mx[:, None])
        ssum = np.zeros(N, T)
        for jj in range(k):
            ssum = ssum + e[:, jj]
        w = e / ssum[:, None]
        g = np.zeros((N, n), T)
        for jj in range(k):
            g = g + gx[:, jj, :n] * w[:, jj, None]
        rate = np.zeros(N, T)
        if c.get("frame"):
            vel = np.asarray(c["vel"]).astype(T)
            for jj in range(k):
                vo = vel[c["row_obs"][:, jj]]
                sj = np.zeros(N, T)
                for cc in range(d - n):
                    sj = sj + gx[:, jj, n + cc] * vo[:, cc]
                rate = rate + sj * w[:, jj]
        distance = dr[:, 0] - T(P["dst_thr"])
        gn = np.sqrt(_sumsq(g, T))
        ghat = g / gn[:, None]
        dot = _dotrows(ghat, vhat, T)
        qo = np.zeros((N, n), T)
        if c.get("frame"):
            fm = T(np.float32(c["frame_max"]))
            r = rate / gn
            r = np.where((gn == 0) | ~(np.abs(r) <= T(FLT_MAX)), T(0), r)
            if mutant != "no_rate_clamp":
                r = np.minimum(np.maximum(r, -fm), fm)
            qo = np.where((gn == 0)[:, None], T(0), -r[:, None] * ghat)
            v = v - qo
            vhat = v / np.sqrt(_sumsq(v, T))[:, None]
            dot = _dotrows(ghat, vhat, T)
            out["ratio"] = rate / gn
        l_vel, l_n, l_tau = _gsig(dot, P["lvel"], T), _gsig(distance, P["ln"], T), _gsig(distance, P["ltau"], T)
        l_nv = l_vel * T(1) + (T(1) - l_vel) * l_n
        ca, va = T(1) - l_n, T(1) - l_vel
        gs = np.zeros(N, T)
        for j in range(n):
            gs = gs + np.sqrt(np.abs(x[:, j]))
        ga_raw = gs * gs
        ga_raw = np.where(ga_raw < 0, T(0), np.where(ga_raw > 1, T(1), ga_raw))
        cut = (ga_raw <= T(P["goal_act_cut"])) if mutant == "cut_le" else (ga_raw < T(P["goal_act_cut"]))
        ga = np.where(cut, T(0), ga_raw)
        act = ca * va * ga
        # RBF policy and the running statistics
        mu, sigma, alpha = s["mu"].astype(T), s["sigma"].astype(T), s["alpha"].astype(T)
        p = T(P["rbf_p"])
        pol = np.zeros((N, n), T)
        phi_all, kval = np.zeros((N, K), T), np.zeros((N, K), T)
        maxact_new = np.array(maxact, dtype=T, copy=True)
        phisum0_new = np.array(phisum0, dtype=T, copy=True)
        for kk in range(K):
            df = q - mu[:, kk, :]
            if P["rbf_p"] == 2:
                nrm = np.sqrt(_sumsq(df, T))
            else:
                sp = np.zeros(N, T)
                for j in range(n):
                    sp = sp + np.abs(df[:, j]) ** p
                nrm = sp ** (T(1) / p)
            phi = np.exp(-sigma[:, kk] * (nrm * nrm))
            phi_all[:, kk] = phi
            kval[:, kk] = phi * act if (int(P["variant"]) & KVAL_TIMES_ACT) else phi
            if not (mutant == "policy_first16" and kk >= 16):
                pol = pol + alpha[:, kk, :] * phi[:, None]
            pa = phi * act
            if i == 1:
                maxact_new[:, kk] = pa
            else:
                old = maxact_new[:, kk]
                maxact_new[:, kk] = np.fmax(old, pa) if mutant == "maxact_fmax" else np.where((old != old) | (pa != pa), T(np.nan), np.fmax(old, pa))
            phisum0_new[kk] = (T(0) if (i == 1 and mutant != "phisum0_no_reset") else phisum0_new[kk]) + phi[0]
        # total velocity, M v, norm clamp, collision, back to the world frame, Euler step
        vt = v + (act[:, None] * pol) * vnorm[:, None]
        gv = _dotrows(ghat, vt, T)
        u = l_tau[:, None] * vt + ((l_nv - l_tau) * gv)[:, None] * ghat
        unorm = np.sqrt(_sumsq(u, T))
        clamped = (unorm < T(P["norm_clamp"])) if mutant == "clamp_lt" else (unorm <= T(P["norm_clamp"]))
        u = u / np.where(clamped, T(1), unorm)[:, None]
        if mutant != "no_nan_to_num":
            u = nan_to_num(u)
        coll = (distance <= 0) if mutant == "coll_le" else (distance < 0)
        rep = (v if mutant == "repulse_v" else ghat * vnorm[:, None]) * T(P["coll_repulse"])
        u = np.where(coll[:, None], u * T(P["coll_slow"]) + rep, u)
        if c.get("frame"):
            u = u + qo
        dq = T(P["dt"]) * u
    out.update(u=u, dq=dq, q_next=(q + dq) if i < c["H"] else None, qdot=u if i == 1 else None, dist=distance, dot=dot, act=act, normal=ghat,
               kval=kval, phi=phi_all, maxact=maxact_new, phisum0=phisum0_new, distance=distance, coll=coll, ga_raw=ga_raw, cut=cut, unorm=unorm,
               clamped=clamped, qo=qo, rate=rate)
    return out


def run(c, T=np.float64, mutant=None):
    """All steps of a case in sequence, the running statistics handed from one to the next -> list of step() results."""
    maxact, phisum0 = c["maxact0"], c["phisum0_0"]
    outs = []
    for s in c["steps"]:
        o = step(c, s, maxact, phisum0, T, mutant)
        maxact, phisum0 = o["maxact"], o["phisum0"]
        outs.append(o)
    return outs


# the thresholds a random row must stay clear of: (branch quantity, threshold, band)
def near_threshold(c, o):
    """[N] bool: the float64 result ``o`` of a step lies within 1e-6 (|u| against norm_clamp: 1e-5) of a branch threshold."""
    P = c["prm"]
    near = (np.abs(o["distance"]) < 1e-6) | (np.abs(o["ga_raw"] - float(P["goal_act_cut"])) < 1e-6) | (np.abs(o["unorm"] - float(P["norm_clamp"])) < 1e-5)
    if "dst" in o:
        near |= np.abs(o["dst"] - float(P["lin_thr"])) < 1e-6
    if "seds_dst" in o:
        near |= (np.abs(o["seds_dst"] - float(np.float32(c["seds"]["lin_thr"]))) < 1e-6) | (np.abs(o["seds_yn"] - float(np.float32(c["seds"]["seds_thr"]))) < 1e-6)
    if "ratio" in o:
        fm = float(np.float32(c["frame_max"]))
        near |= (np.abs(o["ratio"] - fm) < 1e-6) | (np.abs(o["ratio"] + fm) < 1e-6)
    return near
