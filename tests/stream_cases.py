"""The case table of tests/test_gpu_stream_kernels.py and tests/test_cpu_stream_cases.py: the small streaming kernels (scans, replay
ring, running statistics, AdamW / Polyak, Philox fills, policy_act's normaliser) at the sizes where a thread takes a SECOND trip
through its capped grid-stride loop, off 16-byte alignment (the dword fallback behind every 16-byte fast path), and at the scan's
lane-packing edges.

Every cap below restates a launch from the sources (file: function next to it); the predicates (`second_trip`, `scan_kernel`,
`insert_takes_vec`, ...) derive from them which branch a case reaches, and tests/test_cpu_stream_cases.py asserts them without a GPU.

Tolerances.  `gap` of a float32 result against the float64 oracle is max |x32 - x64| / (1 + |x64|), i.e. the smallest t with
|x32 - x64| <= t + t |x64|.  A case keeps its owning module's tolerance (scans 1e-5, statistics 2e-5, policy_act 2e-5: atol = rtol)
while the float32 ORACLE's gap is at most a quarter of it; otherwise its tolerance is 4 x that gap rounded up to one significant
digit, and (gap, tolerance) stand in WIDENED below.  The gap is measured on the references alone, never on a kernel.
"""
import functools
import math

import numpy as np
import torch

from oracle import nets as onets
from oracle import replay as orep
from oracle import scans as oscan

# ------------------------------------------------------------------------------------------------------------------- caps
SCAN_TM_ROWS = 2048 * 256           # scan.hip: launch_scan, time-major: 2048 workgroups x 256 rows (one row per thread)
SCAN_V4_WAVES = 4096 * 4            # scan.hip: launch_scan, k_scan_batch_major_v4: 4096 workgroups x 4 waves, RPW rows per wave
SCAN_BM_WAVES = 2048 * 4            # scan.hip: launch_scan, k_scan_batch_major<TP>: 2048 workgroups x 4 waves, 64/TP rows per wave
INSERT_THREADS = 2048 * 256         # replay.hip: mbpo_replay_insert: one dword (or one 16-byte piece) per thread and trip
GATHER_BLOCKS = 4096                # replay.hip: mbpo_replay_gather / _sample / _sample_mixed: RB rows per workgroup and trip
STATS_BLOCKS = 512                  # replay.hip: STATS_WGS; floor(256 / X) rows per workgroup and trip
GRAD_STATS_ELEMS = 1024 * 256       # optim.hip: ADAMW_MAX_PARTS x 256 (k_grad_stats: block b sums chunks b, b + 1024, ...)
ADAMW_THREADS = 4096 * 256          # optim.hip: ADAMW_MAX_BLOCKS x 256: one quad (16-byte body) or one scalar per thread and trip
SOFT_UPDATE_THREADS = 4096 * 256    # optim.hip: mbpo_soft_update
FILL_THREADS = 4096 * 256           # api.hip: mbpo_philox_normal_fill / _randint_fill / _fill_grouped
NORMALIZE_THREADS = 2048 * 256      # generic_env.hip: mbpo_policy_act -> k_normalize_rows over n * x elements

NAN = float("nan")


def second_trip(items: int, cap: int) -> bool:
    """More items than the capped grid holds at once, not a multiple of it, and the last 256-wide workgroup ragged."""
    return items > cap and items % cap != 0 and items % 256 != 0


def round_up_1sig(x: float) -> float:
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


def gap(x32, x64) -> float:
    x32, x64 = np.asarray(x32, np.float64), np.asarray(x64, np.float64)
    return float((np.abs(x32 - x64) / (1.0 + np.abs(x64))).max())


def within(got, ref, t: float):
    """(ok, worst |got - ref| / (t + t |ref|)); NaN or inf in `got` fails."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ratio = np.abs(got - ref) / (t + t * np.abs(ref))
    worst = float(np.nanmax(ratio)) if ratio.size else 0.0
    return bool(np.isfinite(got).all() and worst <= 1.0), worst


# ----------------------------------------------------------------------------------------------------- alignment helpers
GUARD = 64      # floats of NaN (or sentinel) in front of and behind every guarded view


def misaligned(t: torch.Tensor, k: int, slack=NAN) -> torch.Tensor:
    """A contiguous copy of `t` whose data_ptr() lies k elements (k in 1..3; 0: none) past a 16-byte boundary, cut from a larger
    allocation of 4-byte elements whose other elements (GUARD or more on each side) hold `slack`."""
    assert t.element_size() == 4 and 0 <= k <= 3
    buf = torch.full((t.numel() + 2 * GUARD + 4,), slack, dtype=t.dtype, device=t.device)
    start = GUARD + (k - (buf.data_ptr() // 4) % 4) % 4
    view = buf[start:start + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and (view.data_ptr() // 4) % 4 == k and view.data_ptr() % 4 == 0
    return view


def guarded(shape, dev, k: int = 0, fill=NAN, dtype=torch.float32) -> torch.Tensor:
    """An output for a kernel: `fill` everywhere (NaN, or a sentinel for integers), k elements off alignment, guard bands around it."""
    return misaligned(torch.full(tuple(shape) if not isinstance(shape, int) else (shape,), fill, dtype=dtype, device=dev), k, slack=fill)


def slack_untouched(view: torch.Tensor, slack=NAN) -> bool:
    """The elements of `view`'s allocation outside the view still hold `slack`."""
    whole = torch.empty(0, dtype=view.dtype, device=view.device).set_(view.untyped_storage())
    off, n = view.storage_offset(), view.numel()
    outside = torch.cat([whole[:off], whole[off + n:]])
    assert outside.numel() >= 2 * GUARD
    return bool(torch.isnan(outside).all()) if isinstance(slack, float) and math.isnan(slack) else bool((outside == slack).all())


def aligned16(t: torch.Tensor) -> bool:
    return t.data_ptr() % 16 == 0


# ------------------------------------------------------------------------------------------------------------------ scans
SCAN_TOL = 1e-5                      # tests/test_gpu_replay_scan.py: atol = rtol = 1e-5 against float64; also batch-major vs time-major
GAMMA, LAM = 0.99, 0.95
SCAN_MODES = ("gae", "gae_disc", "lambda")


def scan_kernel(T: int, aligned: bool, time_major: bool = False) -> dict:
    """scan.hip: launch_scan restated: which kernel a batch-major [B, T] scan takes, rows per wave, the wave cap of the grid."""
    if time_major:
        return dict(kernel="tm", rpw=1, waves=SCAN_TM_ROWS, chunks=1)
    if T % 4 == 0 and 8 <= T <= 256 and aligned:
        tl = T // 4
        return dict(kernel="v4", tl=tl, rpw=64 // tl, waves=SCAN_V4_WAVES, chunks=1, idle=64 - tl * (64 // tl))
    tp = 1
    while tp < T and tp < 64:
        tp <<= 1
    return dict(kernel="bm", tp=tp, rpw=64 // tp, waves=SCAN_BM_WAVES, chunks=-(-T // tp))


def scan_groups(B: int, k: dict) -> int:
    return -(-B // k["rpw"])


def _edge_bs(T: int):
    """B = 1, B = RPW - 1 (where RPW > 1) and a B that leaves the last wave group (and the last 4-wave workgroup) ragged."""
    rpw = scan_kernel(T, True)["rpw"]
    bs = [1] + ([rpw - 1] if rpw > 2 else []) + [5 * rpw + rpw // 2]
    return bs


SCAN_CASES = {
    # ---- second trips (every wave / thread beyond the cap is one)
    "tm_2x1048869": dict(T=2, B=2 * 524288 + 256 + 37, tm=True, trip=True),          # k_scan_time_major
    "v4_132x20483": dict(T=132, B=16384 + 4099, trip=True),                         # _v4, TL = 33, RPW = 1, 31 idle lanes
    "bm64_65x16387": dict(T=65, B=2 * 8192 + 3, trip=True),                         # <TP = 64>, two chunks, the later one 1 step
}
for _T in (4, 12, 68, 252, 256, 260):       # <TP=4> | _v4 TL = 3 (RPW 21) | TL = 17 (RPW 3) | TL = 63 | TL = 64 | <64> x 5 chunks, last 4 steps
    for _B in _edge_bs(_T):
        SCAN_CASES[f"edge_{_T}x{_B}"] = dict(T=_T, B=_B)
for _T in (40, 64, 128, 192):               # sizes _v4 owns when aligned: off alignment they take <TP = 64> with 1, 1, 2, 3 chunks
    SCAN_CASES[f"fb_all1_{_T}x11"] = dict(T=_T, B=11, mis="all1")      # every array 1 float past a 16-byte boundary
    SCAN_CASES[f"fb_vs2_{_T}x11"] = dict(T=_T, B=11, mis="vs2")        # only the first output (vs / returns) 2 floats past one
SCAN_CASES["mask_trunc_256x3"] = dict(T=256, B=3, mask="trunc", modes=("gae", "gae_disc"))     # every step truncated
SCAN_CASES["mask_term_256x3"] = dict(T=256, B=3, mask="term", modes=("gae", "gae_disc"))       # every step terminated

# (case, mode) -> (float32-oracle gap, tolerance = 4 x gap rounded up to one digit); everything else keeps SCAN_TOL.
# Measured by tests/test_cpu_stream_cases.py::test_scan_case, which fails when an entry is missing, stale or not needed.
SCAN_WIDENED = {
    ("v4_132x20483", "lambda"): (3.8e-6, 2e-5),       # 0.38 of 1e-5: 132 steps of returns that grow to ~10
    ("bm64_65x16387", "lambda"): (2.9e-6, 2e-5),      # 0.29 of 1e-5
}


def scan_modes(name: str):
    return SCAN_CASES[name].get("modes", SCAN_MODES)


def scan_tol(name: str, mode: str) -> float:
    return SCAN_WIDENED.get((name, mode), (None, SCAN_TOL))[1]


def scan_aligned(case: dict) -> bool:
    return case.get("mis") is None


@functools.lru_cache(maxsize=None)
def scan_inputs(name: str):
    """Time-major [T, B] float32 arrays (the generator of tests/test_gpu_replay_scan.py:_gae_inputs, plus a per-element discount)."""
    c = SCAN_CASES[name]
    T, B = c["T"], c["B"]
    rng = np.random.default_rng(T * 1000 + B)
    trunc = (rng.random((T, B)) < 0.15).astype(np.float32)
    discount = (rng.random((T, B)) > 0.1).astype(np.float32)
    term = ((1 - discount) * (1 - trunc)).astype(np.float32)            # ppo/losses.py:89
    if c.get("mask") == "trunc":
        trunc, term = np.ones((T, B), np.float32), np.zeros((T, B), np.float32)
    if c.get("mask") == "term":
        trunc, term = np.zeros((T, B), np.float32), np.ones((T, B), np.float32)
    inp = dict(trunc=trunc, term=term, rew=rng.standard_normal((T, B)).astype(np.float32),
               val=rng.standard_normal((T, B)).astype(np.float32), boot=rng.standard_normal(B).astype(np.float32),
               disc=np.exp(-0.9 * 0.05 * rng.integers(1, 16, (T, B))).astype(np.float32))
    for a in inp.values():
        a.setflags(write=False)
    return inp


def _scan_oracle(name: str, mode: str, dtype, lam: float = LAM):
    i = scan_inputs(name)
    if mode == "lambda":
        return (oscan.lambda_return(i["rew"], i["val"], GAMMA, lam, dtype=dtype),)
    g = i["disc"] if mode == "gae_disc" else GAMMA
    return oscan.compute_gae(i["trunc"], i["term"], i["rew"], i["val"], i["boot"], g, lam, dtype=dtype)


@functools.lru_cache(maxsize=None)
def scan_oracle64(name: str, mode: str):
    """(vs, adv) or (returns,), time-major float64: computed once, shared, never written again."""
    out = _scan_oracle(name, mode, np.float64)
    for a in out:
        a.setflags(write=False)
    return out


def scan_oracle32(name: str, mode: str):
    return _scan_oracle(name, mode, np.float32)


def td_target(name: str, discounted: bool):
    """lambda = 0: vs is the one-step TD target in closed form (float64)."""
    i = {k: v.astype(np.float64) for k, v in scan_inputs(name).items()}
    v_next = np.concatenate([i["val"][1:], i["boot"][None]], 0)
    g = i["disc"] if discounted else GAMMA
    return (i["rew"] + g * (1 - i["term"]) * v_next - i["val"]) * (1 - i["trunc"]) + i["val"]


# ----------------------------------------------------------------------------------------------------------------- replay
def rows(n: int, D: int, base: float, first: int = 0) -> np.ndarray:
    """n distinct rows: row r, column c holds base + 16 (first + r) + c, exact in float32 (tests/test_gpu_replay_mixed.py:_rows)."""
    out = (base + 16.0 * (first + np.arange(n, dtype=np.float64))[:, None] + np.arange(D, dtype=np.float64)[None, :])
    assert D <= 16 and np.abs(out).max() < 2 ** 24
    return out.astype(np.float32)


def gather_rows_per_block(D: int) -> int:
    """replay.hip: gather_rows_per_block."""
    pieces = D >> 2 if D % 4 == 0 else D
    return max(1, min(256, -(-2048 // pieces)))


def insert_plan(max_size: int, D: int, pos: int, head: int, n: int) -> dict:
    """replay.hip: replay_plan + k_replay_insert's split: physical first row s0, rows before the wrap n1, and the new (pos, head)."""
    roll = min(0, max_size - pos - n)
    p, h = pos + roll, (head - roll) % max_size
    s0 = (p + h) % max_size
    n1 = min(max_size - s0, n)
    return dict(s0=s0, n1=n1, e1=n1 * D, total=n * D, pos=(p + n) % (max_size + 1), head=h)


def insert_takes_vec(plan: dict, D: int, data_k: int = 0, rows_k: int = 0) -> bool:
    """k_replay_insert's `vec`: both copy lengths multiples of 4 floats, and dst1, data and rows on 16-byte boundaries (data_k, rows_k:
    floats past one)."""
    return ((plan["e1"] | plan["total"]) & 3) == 0 and (data_k + plan["s0"] * D) % 4 == 0 and data_k % 4 == 0 and rows_k % 4 == 0


def insert_trips(plan: dict, vec: bool) -> int:
    return -(-(plan["total"] // 4 if vec else plan["total"]) // INSERT_THREADS)


# name: ring rows, D, rows held before (one insert), then the inserts under test; data_k / rows_k: floats off alignment
INSERT_CASES = {
    "big_d12": dict(max=200_000, D=12, held=150_000, batches=[180_000]),          # 16-byte path, wraps, second trip
    # held = 150 001, not 150 000: with 150 000 the 50 000 rows end exactly at the ring's end (no wrap) and both copy lengths are
    # multiples of 4 floats from an aligned start — k_replay_insert would take the 16-byte path in ONE trip (137 500 pieces)
    "big_d11": dict(max=200_000, D=11, held=150_001, batches=[50_000]),           # dword path, wraps, second trip
    "small_d10": dict(max=14, D=10, held=0, batches=[4, 4, 4, 4, 2, 4]),          # 16-byte path at D % 4 != 0, with and without a wrap
    "small_d6": dict(max=14, D=6, held=0, batches=[4, 4, 4, 4, 2, 4]),
    "rows_off_d12": dict(max=64, D=12, held=0, batches=[20, 20, 20, 20, 7], rows_k=1),   # dword path at D % 4 == 0
    "data_off_d12": dict(max=64, D=12, held=0, batches=[20, 20, 20, 20, 7], data_k=3),
}


def insert_plans(case: dict):
    """[(plan, takes_vec, trips)] per insert under test (after the `held` rows)."""
    pos = head = 0
    out = []
    for j, n in enumerate(([case["held"]] if case["held"] else []) + list(case["batches"])):
        p = insert_plan(case["max"], case["D"], pos, head, n)
        pos, head = p["pos"], p["head"]
        if j > 0 or not case["held"]:
            vec = insert_takes_vec(p, case["D"], case.get("data_k", 0), case.get("rows_k", 0))
            out.append((p, vec, insert_trips(p, vec)))
    return out


GATHER_N = GATHER_BLOCKS * 256 + 256 + 77        # with RB = 256: a second trip in two workgroups, the last one ragged
GATHER_RING = dict(max=1000, chunks=(700, 600), sample_position=37)             # wrapped: 1300 distinct rows inserted
# D, n, out_k (floats off alignment); vec: k_replay_gather's 16-byte path
GATHER_CASES = {
    "d4_second_trip": dict(D=4, n=GATHER_N, out_k=0),
    "d3_second_trip": dict(D=3, n=GATHER_N, out_k=0),
    "d12_out_off": dict(D=12, n=600, out_k=2),                                   # dword path at D % 4 == 0
}


def gather_takes_vec(D: int, data_k: int = 0, out_k: int = 0) -> bool:
    return D % 4 == 0 and data_k % 4 == 0 and out_k % 4 == 0


def gather_trips(n: int, D: int) -> int:
    return -(-n // (GATHER_BLOCKS * gather_rows_per_block(D)))


# D / RD, minibatch x G with n_real real rows in front of every minibatch; real_k / out_k: floats off alignment
MIXED_CASES = {
    "12_8": dict(D=12, RD=8, mb=200, G=3, n_real=7),                             # vec_real, the piece at c = 8 zero-filled whole
    "12_8_real_off": dict(D=12, RD=8, mb=200, G=3, n_real=7, real_k=1),          # vec_out, real pieces as four guarded dwords
    "12_11_out_off": dict(D=12, RD=11, mb=200, G=3, n_real=7, out_k=3),          # everything as dwords
    # n = 1 048 575 = 4096 x 256 - 1: every workgroup exactly once, the last one ragged — one row SHORT of a second trip
    "4_3_full_grid": dict(D=4, RD=3, mb=349_525, G=3, n_real=7),
    # n = 1 572 900: a second, ragged trip; the minibatch boundary 2 x 524 300 = 1 048 600 falls 24 rows into workgroup 0's second
    # iteration, so real rows are drawn and zero-padded there
    "4_3_second_trip": dict(D=4, RD=3, mb=524_300, G=3, n_real=7),
}
MIXED_RINGS = dict(model=dict(max=1000, chunks=(700, 600), sample_position=37), real=dict(max=23, chunks=(15, 15), sample_position=2))
SEED, OFF, ROFF = 2 ** 40 + 7, (2 << 32) + 5, (3 << 32) + 5


def ring_chunks(ring: dict, D: int, base: float):
    out, first = [], 0
    for n in ring["chunks"]:
        out.append(rows(n, D, base, first))
        first += n
    return out


def oracle_ring(ring: dict, D: int, base: float):
    """(queue, state) of the oracle after the ring's inserts, with its sample_position written afterwards (inserts alone leave 0)."""
    q = orep.UniformSamplingQueue(ring["max"], D, 1)
    st = q.init()
    for c in ring_chunks(ring, D, base):
        st = q.insert(st, c)
    return q, dict(st, sample_position=np.int32(ring["sample_position"]))


# ----------------------------------------------------------------------------------------------------- running statistics
STATS_TOL = 2e-5                     # tests/test_gpu_replay_scan.py::test_running_stats
STATS_CASES = {
    "x4": dict(X=4, D=12, off=0, n=2 * 32768 + 197),          # 64 rows per trip and workgroup: second trip
    "x128": dict(X=128, D=128, off=0, n=2051),                # two rows per trip
    "x100": dict(X=100, D=103, off=3, n=2500),                # two rows per trip, 56 idle threads per workgroup
    "x17": dict(X=17, D=43, off=5, n=3 * 7680 + 11),          # 15 rows per trip, one idle thread
}
# name -> (float32-oracle gap, tolerance): the float32 oracle adds 65 733 (23 051) terms one after the other
STATS_WIDENED = {
    "x4": (1.7e-5, 7e-5),                             # 0.81 of 2e-5
    "x17": (7.1e-6, 3e-5),                            # 0.35 of 2e-5
}


def stats_tol(name: str) -> float:
    return STATS_WIDENED.get(name, (None, STATS_TOL))[1]


def stats_rows_per_trip(X: int) -> int:
    return STATS_BLOCKS * (256 // X)


@functools.lru_cache(maxsize=None)
def stats_batches(name: str):
    c = STATS_CASES[name]
    rng = np.random.default_rng(2)
    out = tuple((rng.standard_normal((c["n"], c["D"])) * 3 + 1.5).astype(np.float32) for _ in range(3))
    for a in out:
        a.setflags(write=False)
    return out


def stats_ref64(name: str, stats: np.ndarray, it: int) -> np.ndarray:
    c = STATS_CASES[name]
    b = stats_batches(name)[it][:, c["off"]:c["off"] + c["X"]]
    return orep.stats_update(stats.astype(np.float64), b.astype(np.float64), dtype=np.float64)


# -------------------------------------------------------------------------------------------------------- AdamW / Polyak
ADAMW_LR, ADAMW_WD, ADAMW_TAU = 3e-3, 1e-2, 0.05      # tests/test_gpu_bptt.py::test_adamw_step_parity
ADAMW_CASES = {
    "grad_stats_trip": dict(n=262_144 + 1_000 + 3),                     # k_grad_stats: chunks 1024 .. 1027 on a second trip; tail of 3
    "body_trip": dict(n=4_194_304 + 1_024 + 2),                         # 16-byte body: 256 quads on a second trip; tail of 2
    "target_off": dict(n=1_048_576 + 301, target_k=1),                  # nq = 0: everything on the scalar path, second trip
}
SOFT_UPDATE_N = 1_048_576 + 257


def adamw_quads(case: dict) -> int:
    """k_adamw_step's nq."""
    return 0 if case.get("target_k") else case["n"] >> 2


# ------------------------------------------------------------------------------------------------------------ Philox fills
NORMAL_TOL = 2e-6                    # tests/test_gpu_bptt_generic.py::test_philox_normal_fill_is_the_kernels_stream
FILL_N = 1_048_576 + 300
# the element index elem_base + i passes 2^32 at i = 100 (first trip) and at i = 1 048 676 (second trip)
FILL_BASES = {"wrap_in_first_trip": 2 ** 32 - 100, "wrap_in_second_trip": 2 ** 32 - (FILL_THREADS + 100)}
GROUPED = dict(S=3, B=5, G=70_001, seeds=(0x1234, (1 << 64) - 5, 42, 2 ** 40 + 9, 7))


# -------------------------------------------------------------------------------------------------------------- policy_act
ACT_TOL = 2e-5                       # tests/test_gpu_generic_system.py::test_policy_act_matches_oracle_and_bad_shapes (log_prob: 5e-5)
ACT_LP_TOL = 5e-5
ACT = dict(X=4, U=1, dims=[4, 64, 64, 2], n=131_072 + 300)
ACT_WIDENED = {
}


def act_tol(what: str) -> float:
    return ACT_WIDENED.get(what, (None, ACT_LP_TOL if what == "log_prob" else ACT_TOL))[1]


@functools.lru_cache(maxsize=None)
def act_inputs():
    g = torch.Generator().manual_seed(11)
    n, X, U = ACT["n"], ACT["X"], ACT["U"]
    return dict(ppar=onets.init_mlp_flat(ACT["dims"], g), obs=torch.randn(n, X, generator=g) * 1.5 + 0.3,
                nm=torch.randn(X, generator=g) * 0.3, ns=torch.rand(X, generator=g) + 0.5, noise=torch.randn(n, U, generator=g))


def act_oracle(dtype):
    """dict(mode, raw, action, log_prob) of the oracle's MLP and NormalTanh head."""
    i = {k: v.to(dtype) for k, v in act_inputs().items()}
    logits = onets.mlp_forward(i["ppar"], ACT["dims"], onets.normalize(i["obs"], i["nm"], i["ns"]), "swish")
    z = onets.sample_no_postprocessing(logits, i["noise"])
    return dict(mode=onets.mode(logits), raw=z, action=onets.postprocess(z), log_prob=onets.log_prob(logits, z))


@functools.lru_cache(maxsize=None)
def act_oracle64():
    return act_oracle(torch.float64)
