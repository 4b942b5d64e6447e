"""The per-rollout modulation step (csrc/step_device.h: modulate_core) on the device, ONE step at a time on caller-supplied inputs
(omds_test_modulate, include/omds_test.h), against the float64 reference tests/step_ref.py on the cases of tests/step_edge_cases.py:
every shape, every designed row that sits exactly on a branch, the non-finite semantics provoked on purpose, both lane counts
(nsub = 1: k_modulate through the production launcher; nsub = 16: modulate_core as the fused step kernels call it).
tests/test_step_edges_cpu.py pins the reference, shows that float32 can meet the bars on these inputs, that the cases catch eleven
mutants, and that no random row is excluded (the 1e-6 bands around the branch thresholds hold 0 of 4994 random rows).

Bars (step_edge_cases.compare): helpers.RTOL = 1e-5 of the largest reference magnitude of the output in the case for qdot,
q_next - q, normal, dot, act, kval, maxact and phisum0; 1e-6 absolute for the distance; the non-finite pattern of every output, the
0xFFFFFFFF of what a step leaves alone (trajT at step == H, qdot behind step 1, kval / maxact / phisum0 from K on) and the
bit-identity cases exactly.  One class cannot meet RTOL of its own scale, activations that are below 0.048 in the whole case: 4 x
2^-23 absolute there (step_edge_cases.ACT_ATOL; the float32 restatement's worst error on the class is 8.9e-8).

Worst error / bar over all cases (1.0 = the bar), as both modules print them:

  output    float32 restatement (CPU)   device, nsub = 1   device, nsub = 16
  qdot              0.188                    0.182               0.073
  q_next - q        0.469                    0.469               0.175      (seds_G2_strong: the row at q = 60, where ulp(q) = 3.8e-6)
  normal            0.125                    0.055               0.055
  dot               0.146                    0.040               0.040
  act               0.188                    0.130               0.130
  kval              0.201                    0.101               0.101
  maxact            0.201                    0.101               0.101
  phisum0           0.062                    0.062               0.062
  distance          0.015                    0.015               0.015
  (nsub = 16 runs neither SEDS nor n_dof other than 2 and 7, hence its smaller maxima.)

The lane-count identity HELD: for K = 0 and K = 1 (n_dof 2 and 7, frame on and off) every output of the 16-lane form is the 1-lane
form's bit for bit, and for K >= 2 everything but qdot / q_next is.  The frame at rest returned the bits of the plain step on every
case tried, both lane counts, NaN rows included.  No test exposed a bug in step_device.h."""
import numpy as np
import pytest

import step_edge_cases as sec
import step_ref as sr

pytestmark = pytest.mark.gpu
F32 = np.float32
SENT = 0xFFFFFFFF
_CACHE = {}


def cases():
    if not _CACHE:
        _CACHE["cases"] = {c["name"]: c for c in sec.all_cases()}
        _CACHE["refs"] = {}
        _CACHE["dev"] = {}
    return _CACHE["cases"]


def reference(c):
    cases()
    if c["name"] not in _CACHE["refs"]:
        _CACHE["refs"][c["name"]] = sr.run(c)
    return _CACHE["refs"][c["name"]]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def device(c, nsub):
    """All steps of a case through the hook, the running statistics handed from one step to the next as the device left them
    -> list of the hook's raw results (float32 arrays in the reference's layouts)."""
    from optimalmodulationds_amd import _lib
    cases()
    key = (c["name"], nsub)
    if key not in _CACHE["dev"]:
        maxact, phisum0, outs = c["maxact0"], c["phisum0_0"], []
        for s in c["steps"]:
            r = _lib.modulate_step(nsub=nsub, step=s["step"], H=c["H"], prm=sec.to_params(c["prm"]), qf=c["qf"], q=s["q"], drow=c["drow"], gradx=c["gradx"],
                                   mu=s["mu"], sigma=s["sigma"], alpha=s["alpha"], Kmax=c["Kmax"], maxact=maxact, phisum0=phisum0, A=c["A"],
                                   seds=c["seds"], frame=c["frame"], frame_max=float(c["frame_max"]), vel=c["vel"], row_obs=c["row_obs"])
            maxact, phisum0 = r["maxact"], r["phisum0"]
            outs.append(r)
        _CACHE["dev"][key] = outs
    return _CACHE["dev"][key]


def device_outputs(c, s, r, maxact_in, phisum0_in):
    """The hook's raw result as step_edge_cases.reference_outputs lays a step out, after the EXACT checks on what a step must leave
    alone: trajT[step] at step == H, qdot behind step 1, kval from K on (all still 0xFFFFFFFF), maxact / phisum0 from K on (the bits
    they came in with); and nothing the step writes still holds the fill pattern."""
    K, i = c["K"], s["step"]
    f = lambda a: np.asarray(a, np.float64)
    written = [r["dist"], r["dot"], r["act"], r["normal"], r["kval"][:, :K], r["maxact"][:, :K], r["phisum0"][:K]]
    if i < c["H"]:
        written.append(r["q_next"])
    else:
        assert (bits(r["q_next"]) == SENT).all(), "step == H wrote the rollouts"
    if i == 1:
        written.append(r["qdot"])
    else:
        assert (bits(r["qdot"]) == SENT).all(), "a step behind the first wrote qdot"
    assert (bits(r["kval"][:, K:]) == SENT).all(), "kernel values written from K on"
    assert np.array_equal(bits(r["maxact"][:, K:]), bits(maxact_in[:, K:])) and np.array_equal(bits(r["phisum0"][K:]), bits(phisum0_in[K:])), "statistics touched from K on"
    for a in written:
        assert not (bits(a) == SENT).any(), "an output the step must write still holds the fill pattern"
    return dict(qdot=f(r["qdot"]) if i == 1 else None, dq=f(r["q_next"]) - f(s["q"]) if i < c["H"] else None, normal=f(r["normal"]), dot=f(r["dot"]),
                act=f(r["act"]), kval=f(r["kval"][:, :K]), maxact=f(r["maxact"][:, :K]), phisum0=f(r["phisum0"][:K]), dist=f(r["dist"]))


ALL = [(c["name"], nsub) for c in sec.all_cases() for nsub in c["nsubs"]]


@pytest.mark.parametrize("name,nsub", ALL, ids=[f"{n}-{s}" for n, s in ALL])
def test_step_against_the_reference(name, nsub):
    c = cases()[name]
    refs, raws = reference(c), device(c, nsub)
    gots, maxact, phisum0 = [], c["maxact0"], c["phisum0_0"]
    for s, r in zip(c["steps"], raws):
        gots.append(device_outputs(c, s, r, maxact, phisum0))
        maxact, phisum0 = r["maxact"], r["phisum0"]
    e = sec.errors(c, refs, gots)
    print(f"{name} nsub {nsub}: error / bar " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(e.items())))
    assert max(e.values()) <= 1.0, f"{name} nsub {nsub}: error / bar {e}"
    # the exact outcomes a designed row can show in its outputs: the distance on the threshold, the activation cut to 0
    for row, exp in c["expect"].items():
        if "distance" in exp:
            assert raws[0]["dist"][row] == F32(exp["distance"])
        if exp.get("cut"):
            assert raws[0]["act"][row] == 0 or np.isnan(raws[0]["act"][row])
        if exp.get("cut") is False:
            assert raws[0]["act"][row] != 0


def _same_bits(ra, rb, names=("q_next", "qdot", "dist", "dot", "act", "normal", "kval", "maxact", "phisum0")):
    """The outputs that differ in bits between two raw results (a NaN equals a NaN: its sign and payload are not results), each with
    its first differing entries."""
    diff = []
    for n in names:
        a, b = np.asarray(ra[n], F32), np.asarray(rb[n], F32)
        ne = (bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))
        if ne.any():
            where = np.argwhere(ne)[:4]
            diff.append((n, [(tuple(int(x) for x in w), float(a[tuple(w)]), float(b[tuple(w)])) for w in where]))
    return diff


LANES = [c["name"] for c in sec.lane_cases()]


@pytest.mark.parametrize("name", LANES)
def test_lane_counts_against_each_other(name):
    """K <= 1: 16 lanes per rollout perform the operations of one lane in the same order (the policy sum has at most one term, the
    shuffles add zeros): every output bit-identical.  K >= 2: only the policy sum is ordered differently, so everything that does not
    depend on it is bit-identical still, and qdot / q_next meet the bars against the reference (test_step_against_the_reference)."""
    c = cases()[name]
    (r1,), (r16,) = device(c, 1), device(c, 16)
    if c["K"] <= 1:
        assert not _same_bits(r1, r16), f"{name}: differ in bits between the lane counts: {_same_bits(r1, r16)}"
    else:
        independent = ("dist", "dot", "act", "normal", "kval", "maxact", "phisum0")
        assert not _same_bits(r1, r16, independent), f"{name}: {_same_bits(r1, r16, independent)}"


AT_REST = [n for n in LANES if n.endswith("_f0")] + [f"{k}_n{n}" for n in (2, 7) for k in ("nominal", "collision", "goal", "policy_p3_v0", "blend")]


@pytest.mark.parametrize("name", AT_REST)
def test_frame_at_rest_returns_the_bits_of_the_plain_step(name):
    """With every obstacle velocity zero the FRAME instantiation returns the bits of the plain one (step_device.h: with qo = 0 every
    operation returns its operand), for both lane counts -- the NaN rows of the designed cases included."""
    c = cases()[name]
    rest = sec.at_rest(c)
    for nsub in c["nsubs"]:
        (plain,), (framed,) = device(c, nsub), device(rest, nsub)
        assert not _same_bits(plain, framed), f"{name} nsub {nsub}: the frame at rest differs in {_same_bits(plain, framed)}"


def test_statistics_are_overwritten_at_step_1_and_summed_after():
    """maxact and phisum0 hold garbage before step 1 of the sequence cases: step 1 overwrites them; phisum0 after steps 1..3 is the sum
    over the steps of rollout 0's kernel values; maxact is NaN from step 2 on for kernel 1 of rollout 2 (its sigma is NaN at step 2),
    and for nothing else."""
    for n in (2, 7):
        c = cases()[f"sequence_n{n}"]
        K = c["K"]
        for nsub in c["nsubs"]:
            r1, r2, r3 = device(c, nsub)
            assert np.array_equal(bits(r1["phisum0"][:K]), bits(r1["kval"][0, :K])), "phisum0 after step 1 is rollout 0's kernel values"
            want = (r1["kval"][0, :K] + r2["kval"][0, :K]) + r3["kval"][0, :K]
            assert np.array_equal(bits(r3["phisum0"][:K]), bits(want)), "phisum0 after step 3 is the sum over the steps, in step order"
            for r, nan_now in ((r1, False), (r2, True), (r3, True)):
                m = np.isnan(r["maxact"][:, :K])
                assert m[2, 1] == nan_now and m.sum() == int(nan_now)
            assert (r1["maxact"][:, :K] <= 1).all(), "the garbage (5..9) is gone"
