"""The trainer's route and split policy (optimalmodulationds_amd/csrc/train_plan_def.h: which kernel multiplies each of a layer's three
products, how the contractions over the batch are cut) on the host: no library, no GPU.  tests/train_plan_host.cpp, a stand-alone
program around the header train.hip includes, is built under AddressSanitizer + UBSan and prints the plan of every (dims, B) here.

(a) every case of tests/test_gpu_train_grad.py and the shapes of tests/test_gpu_train.py's special-shape test reach, layer by layer,
    the routes of `restate_routes` -- the rules restated here in the order the trainer asks them, written from the trainer's code
    as it stood before the header existed, not from the header (EXPERIMENTS.md R24) -- and the routes their comments name; with
    the general-kernel flag every route is general;
(b) the split numbers are pinned as literals, computed once from the same arithmetic;
(c) each predicate has one case on each side of each of its edges."""
import inspect
import struct
import subprocess

import pytest

import test_gpu_train
import test_gpu_train_grad
from helpers import sanitized_host_program

NONE, GENERAL, TALL, THIN, THIN_OUT, WGRAD_FIRST, WGRAD_LAST = range(7)      # enum TrainRoute
SHIPPED = [30, 256, 256, 256, 256, 9]


def restate_routes(dims, general):
    """[(forward, wgrad, wgrad_tt, inputgrad)] per layer, in the order the trainer asked its launchers"""
    rows = []
    for i, (n_in, n_out) in enumerate(zip(dims[:-1], dims[1:])):
        def thin(N, K):                      # launch_gemm_thin: K > THIN_KMAX || N > 256 || N < 64 || thin_off() -> "not me"
            return not (K > 32 or N > 256 or N < 64 or general)

        def tall(N, K):                      # tall_shape(N, K), then launch_gemm_tall's own reject (lda == K here)
            return N > 128 and N <= 256 and K == 256 and not general

        if thin(n_out, n_in):
            fwd = THIN
        elif n_out <= 16 and n_in <= 256 and n_in > 32 and not general:
            fwd = THIN_OUT
        elif tall(n_out, n_in):
            fwd = TALL
        else:
            fwd = GENERAL
        if n_in <= 32 and n_out <= 4096 and n_out > 32 and not general:
            wg, T = WGRAD_FIRST, n_in
        elif n_out <= 32 and n_in <= 4096 and n_in > 32 and not general:
            wg, T = WGRAD_LAST, n_out
        else:
            wg, T = GENERAL, None
        tt = 0 if T is None else 4 if T <= 4 else 12 if T <= 12 else 16 if T <= 16 else 32
        if i == 0:
            ig = NONE
        elif thin(n_in, n_out):
            ig = THIN
        elif tall(n_in, n_out):
            ig = TALL
        else:
            ig = GENERAL
        rows.append((fwd, wg, tt, ig))
    return rows


def restate_split(B, n_in, n_out, partial_floats):
    """(splits, kchunk, rows of the last chunk, rsplit, rows_per): omds_trainer_step's arithmetic, TM = TN = 128, TK = 16"""
    tiles = ((n_out + 127) // 128) * ((n_in + 127) // 128)
    splits = max(1, min(256, 1024 // max(tiles, 1), (B + 63) // 64))
    while splits * n_out * n_in > partial_floats:
        splits -= 1
    kchunk = ((B + splits - 1) // splits + 15) // 16 * 16
    splits = (B + kchunk - 1) // kchunk
    rsplit = max(1, min(2048, B // 256, partial_floats // n_out))
    return splits, kchunk, B - (splits - 1) * kchunk, rsplit, (B + rsplit - 1) // rsplit


def _gpu_cases():
    """(id, dims, B) of the GPU tests whose comments name routes"""
    cases = [(cid, list(dims), B) for cid, dims, _, B, _ in test_gpu_train_grad.CASES]
    fn = test_gpu_train.test_special_shape_kernels_are_the_general_kernel_bit_for_bit
    assert "SdfTrainer([30, 256, 256, 256, 256, 9], act" in inspect.getsource(fn)
    (mark,) = [m for m in fn.pytestmark if m.name == "parametrize"]
    cases += [(f"special-{act}-B{B}", SHIPPED, B) for act, B in mark.args[1]]
    return cases


# What the comments of tests/test_gpu_train_grad.py say each case reaches, per layer: (forward, wgrad, wgrad_tt, inputgrad)
_FIRST, _HIDDEN, _LAST = (THIN, WGRAD_FIRST, 32, NONE), (TALL, GENERAL, 0, TALL), (THIN_OUT, WGRAD_LAST, 12, THIN)
NAMED = {
    "C1": [_FIRST, _HIDDEN, _HIDDEN, _HIDDEN, _LAST],
    "C6": [_FIRST, _HIDDEN, _HIDDEN, _HIDDEN, _LAST],
    "C9-franka": [_FIRST, _HIDDEN, _HIDDEN, _HIDDEN, _LAST],
    "special": [_FIRST, _HIDDEN, _HIDDEN, _HIDDEN, _LAST],
    "C2-planar2": [(THIN, WGRAD_FIRST, 16, NONE), _HIDDEN, _HIDDEN, _HIDDEN, (THIN_OUT, WGRAD_LAST, 4, THIN)],
    "C3": [(THIN, WGRAD_FIRST, 12, NONE), _HIDDEN, (THIN_OUT, WGRAD_LAST, 4, THIN)],
    # 256 -> N: tall forward, k_gemm input gradient; N -> 256: k_gemm forward, tall input gradient
    "C4": [_FIRST, (TALL, GENERAL, 0, GENERAL), (GENERAL, GENERAL, 0, TALL), _LAST],
    # 256 -> 20: k_gemm forward (20 > THINN_NMAX), last-layer form, thin input gradient; 20 -> 256: thin forward, first-layer form
    "C5": [_FIRST, (GENERAL, WGRAD_LAST, 32, THIN), (THIN, WGRAD_FIRST, 32, GENERAL), _LAST],
    "C7": [(GENERAL, GENERAL, 0, NONE), (GENERAL, GENERAL, 0, GENERAL), (GENERAL, WGRAD_LAST, 32, THIN)],
    "C8-64-63-16": [_FIRST, (GENERAL, GENERAL, 0, GENERAL), (THIN_OUT, WGRAD_LAST, 16, GENERAL)],
    "C8-300-129": [(GENERAL, WGRAD_FIRST, 32, NONE), (GENERAL, GENERAL, 0, GENERAL), _LAST],
    "C8-300-257": [(GENERAL, WGRAD_FIRST, 32, NONE), (GENERAL, GENERAL, 0, GENERAL), (GENERAL, WGRAD_LAST, 12, GENERAL)],
}

# (b): (splits, kchunk, rows of the last chunk, rsplit, rows_per), the same for every layer of the case
PINS = [
    (SHIPPED, 1, (1, 16, 1, 1, 1)),
    (SHIPPED, 63, (1, 64, 63, 1, 63)),
    (SHIPPED, 65, (2, 48, 17, 1, 65)),
    (SHIPPED, 257, (5, 64, 1, 1, 257)),
    (SHIPPED, 3001, (47, 64, 57, 11, 273)),
    (SHIPPED, 49153, (237, 208, 65, 192, 257)),
    ([12, 256, 256, 4], 300, (5, 64, 44, 1, 300)),
    ([30, 300, 257, 9], 129, (3, 48, 33, 1, 129)),
]

# (c): (dims, layer, field, value) -- field 0 forward, 1 wgrad, 2 wgrad_tt, 3 inputgrad; the two sides of an edge stand together
EDGES = [
    # k_gemm_thin forward: 64 <= out <= 256, in <= 32
    ([30, 63, 9], 0, 0, GENERAL), ([30, 64, 9], 0, 0, THIN), ([30, 256, 9], 0, 0, THIN), ([30, 257, 9], 0, 0, GENERAL),
    ([30, 32, 128, 9], 1, 0, THIN), ([30, 33, 128, 9], 1, 0, GENERAL),
    # k_gemm_thin_out: out <= 16, 32 < in <= 256
    ([30, 200, 16], 1, 0, THIN_OUT), ([30, 200, 17], 1, 0, GENERAL), ([30, 32, 16], 1, 0, GENERAL), ([30, 33, 16], 1, 0, THIN_OUT),
    ([30, 256, 16], 1, 0, THIN_OUT), ([30, 257, 16], 1, 0, GENERAL),
    # k_gemm_tall forward: in == 256, 128 < out <= 256
    ([30, 256, 128, 9], 1, 0, GENERAL), ([30, 256, 129, 9], 1, 0, TALL), ([30, 255, 256, 9], 1, 0, GENERAL), ([30, 256, 256, 9], 1, 0, TALL),
    ([30, 257, 256, 9], 1, 0, GENERAL), ([30, 256, 257, 9], 1, 0, GENERAL),
    # input gradient: thin out <= 32 and 64 <= in <= 256; tall out == 256 and 128 < in <= 256
    ([30, 64, 32, 9], 1, 3, THIN), ([30, 64, 33, 9], 1, 3, GENERAL), ([30, 63, 32, 9], 1, 3, GENERAL), ([30, 256, 32, 9], 1, 3, THIN),
    ([30, 257, 32, 9], 1, 3, GENERAL), ([30, 128, 256, 9], 1, 3, GENERAL), ([30, 129, 256, 9], 1, 3, TALL), ([30, 256, 255, 9], 1, 3, GENERAL),
    ([30, 256, 256, 9], 1, 3, TALL), ([30, 256, 9], 0, 3, NONE),
    # weight gradient: in <= 32 < out <= 4096 (first-layer form), out <= 32 < in <= 4096 (last-layer form)
    ([30, 32, 9], 0, 1, GENERAL), ([30, 33, 9], 0, 1, WGRAD_FIRST), ([30, 32, 128, 9], 1, 1, WGRAD_FIRST), ([30, 33, 128, 9], 1, 1, GENERAL),
    ([30, 128, 32], 1, 1, WGRAD_LAST), ([30, 128, 33], 1, 1, GENERAL), ([30, 4096, 9], 0, 1, WGRAD_FIRST), ([30, 4096, 9], 1, 1, WGRAD_LAST),
    ([30, 4097, 9], 0, 1, GENERAL), ([30, 4097, 9], 1, 1, GENERAL),      # (omds_trainer_create refuses 4097: only that no thin form is chosen)
    # k_wgrad_thin's instantiation by the thin width T
    ([30, 256, 4], 1, 2, 4), ([30, 256, 5], 1, 2, 12), ([30, 256, 12], 1, 2, 12), ([30, 256, 13], 1, 2, 16), ([30, 256, 16], 1, 2, 16),
    ([30, 256, 17], 1, 2, 32), ([3, 256, 9], 0, 2, 4), ([6, 256, 9], 0, 2, 12), ([12, 256, 9], 0, 2, 12), ([15, 256, 9], 0, 2, 16),
    ([18, 256, 9], 0, 2, 32), ([30, 256, 256, 9], 1, 2, 0),
]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan(dims, B, general=0) -> [(forward, wgrad, wgrad_tt, inputgrad, splits, kchunk, last rows, rsplit, rows_per)] per layer, from
    ONE run of the sanitized program over every (dims, B, general) this module asks about"""
    tmp = tmp_path_factory.mktemp("train_plan")
    exe = sanitized_host_program("train_plan_host", tmp)
    asks = [(d, B, g) for _, d, B in _gpu_cases() for g in (0, 1)] + [(d, B, 0) for d, B, _ in PINS] + [(d, 257, g) for d, _, _, _ in EDGES for g in (0, 1)]
    asks = sorted({(tuple(d), B, g) for d, B, g in asks})
    fin, fout = tmp / "cases.bin", tmp / "out.bin"
    fin.write_bytes(struct.pack("<i", len(asks)) + b"".join(struct.pack(f"<iii{len(d)}i", g, len(d) - 1, B, *d) for d, B, g in asks))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "train_plan_host: done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    raw, off, table = fout.read_bytes(), 0, {}
    for d, B, g in asks:
        table[(d, B, g)] = [struct.unpack_from("<9i", raw, off + 36 * i) for i in range(len(d) - 1)]
        off += 36 * (len(d) - 1)
    assert off == len(raw)
    return lambda dims, B, general=0: table[(tuple(dims), B, general)]


CASES = _gpu_cases()


@pytest.mark.parametrize("cid,dims,B", CASES, ids=[c[0] for c in CASES])
def test_every_gpu_case_reaches_the_routes_it_names(plan, cid, dims, B):
    pf = 256 * max(a * b for a, b in zip(dims[:-1], dims[1:]))
    for general in (0, 1):
        got = plan(dims, B, general)
        assert [g[:4] for g in got] == restate_routes(dims, general), (cid, general)
        assert [g[4:] for g in got] == [restate_split(B, a, b, pf) for a, b in zip(dims[:-1], dims[1:])], (cid, general)
    assert all(g[:4] == (GENERAL, GENERAL, 0, GENERAL if i else NONE) for i, g in enumerate(plan(dims, B, 1)))
    (name,) = [k for k in NAMED if cid == k or cid.startswith(k + "-")]
    assert [g[:4] for g in plan(dims, B)] == NAMED[name], cid


def test_the_gpu_cases_cover_every_route_and_instantiation(plan):
    seen = [g[:4] for _, dims, B in CASES for g in plan(dims, B)]
    assert {s[0] for s in seen} == {GENERAL, TALL, THIN, THIN_OUT}
    assert {s[1:3] for s in seen} >= {(GENERAL, 0)} | {(f, tt) for f in (WGRAD_FIRST, WGRAD_LAST) for tt in (12, 16, 32)} | {(WGRAD_LAST, 4)}
    assert {s[3] for s in seen} == {NONE, GENERAL, TALL, THIN}


@pytest.mark.parametrize("dims,B,want", PINS, ids=[f"{len(d) - 1}x{d[1]}-B{B}" for d, B, _ in PINS])
def test_split_numbers_are_pinned(plan, dims, B, want):
    assert [g[4:] for g in plan(dims, B)] == [want] * (len(dims) - 1)


def test_route_edges(plan):
    for dims, layer, field, want in EDGES:
        assert plan(dims, 257)[layer][field] == want, (dims, layer, field)
        assert plan(dims, 257)[layer][:4] == restate_routes(dims, 0)[layer]
        assert plan(dims, 257, 1)[layer][:4] == (GENERAL, GENERAL, 0, GENERAL if layer else NONE)
