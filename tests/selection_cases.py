"""Inputs for the kernels that turn logits into token ids: the two greedy kernels (k_argmax_advance, k_batch_argmax; csrc/kernels_llama.h) and the
sampler kernels (k_sample<32|64>, k_sample_small<32|64>; csrc/kernels_sample.h).  Plain numpy, no GPU: tests/test_selection_cases_cpu.py holds the
checker to the references on exactly these inputs, tests/test_gpu_selection.py holds the kernels to them.

Greedy rows.  The expected id is the checker's rule (oracle/oracle.c argmax_f32, the reference's generation loop): best = 0; for i in 1..: if
x[i] > x[best]: best = i - strict >, so the lowest index wins a tie, a NaN at index 0 wins the row and a NaN anywhere else is never taken.
rule_argmax restates it (np.argmax treats NaN differently and is not used).  Where a row's id is known by construction it is carried along and the
CPU test holds the rule to it.  The positions follow how the kernels hand out ids: k_batch_argmax (and k_argmax_advance on rows that are not
16-byte aligned or whose length is no multiple of 4) gives thread t the ids t, t + 1024, ...; k_argmax_advance otherwise gives thread t the ids
4 (t + 1024 u) .. + 3 (u = 0, 1, ...; four u per sweep, so id 16384 opens the second sweep).  Lanes 63 | 64 are a wave edge, threads 0..63 and
960..1023 the first and the last of the 16 waves.

Sampler cases.  (logits, ring, topK, topP, temp, penalty), two draws each; the reference is tests/sampler_ref.py.  NaN logits are NOT in scope for
the sampler: the reference sorts by value, and a sort over NaN is unspecified (the Go original's sort.Slice and numpy's lexsort order them
differently), so no expected output exists.  +inf logits are in scope: inf - inf makes every probability NaN, identically everywhere, and the
candidates' order and the token are still defined - compare probabilities with equal_nan."""
import numpy as np

import sampler_ref

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
DENORM = np.float32(1.4e-45)

ARGMAX_V = (1, 3, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 32000, 32001, 32002, 32003, 65535, 65536)


def rule_argmax(x):
    """The checker's loop, restated (vectorised: a Python loop over 65536 x 100 rows x 20 sizes is minutes): a NaN at 0 is never beaten; otherwise
    x[best] is never NaN, `x[i] > x[best]` skips every NaN, and the first index of the maximum of the rest is where the loop ends."""
    if x[0] != x[0]:
        return 0
    return int(np.flatnonzero(x == np.nanmax(x))[0])


def rule_argmax_loop(x):
    """The rule word for word (the CPU test holds rule_argmax to it on the rows short enough for a Python loop)."""
    best = 0
    for i in range(1, len(x)):
        if x[i] > x[best]:
            best = i
    return best


# ids at which one maximum / the members of a tie are placed (those that exist for a given V)
SINGLE_IDS = (0, 1, 2,                      # the row's first three ids (the last three are added per V)
              4, 5, 6, 7,                   # the four elements of one float4
              63, 64,                       # lane 63 | 64 of wave 0, one id per thread
              252, 255, 256,                # the same wave edge with four ids per thread
              959, 960, 1023, 1024, 1028,   # wave 14 | 15, the last thread, a thread's second element (one id per thread)
              3836, 3840, 4092, 4095, 4096, 4100,   # the same with four ids per thread (4096: thread 0 again)
              16383, 16384, 16388,          # the second sweep of 4096 float4
              20000, 31999)
TIES = ((5, 1029), (5, 1029, 2053),         # one thread of k_batch_argmax
        (8, 9), (8, 16392), (8, 9, 16392), (8, 11, 4104),   # one thread of k_argmax_advance (same float4, next sweep, next u)
        (10, 11), (8, 12), (10, 11, 12),    # adjacent lanes under either mapping
        (63, 64), (252, 256), (255, 256), (62, 63, 64),     # the wave edge
        (1023, 1024), (4095, 4096),         # the last thread against thread 0's next element: the LOWER id sits in the HIGHER thread
        (3, 1000), (3, 4000), (3, 500, 1000),               # first and last wave
        (700, 16384), (1, 40000, 65535))


def argmax_rows(V):
    """-> (X float32 [n][V], names [n], known [n]: the id by construction or None).  Deterministic."""
    rng = np.random.default_rng(1000 + V)
    rows, names, known = [], [], []

    def add(name, x, want=None):
        assert x.shape == (V,) and x.dtype == np.float32
        rows.append(x); names.append(name); known.append(want)

    def noise():    # distinct-ish finite values well below the planted ones
        return (rng.standard_normal(V) * 0.5).clip(-3, 3).astype(f32)

    add("rising", np.arange(V, dtype=f32), V - 1)
    add("falling", -np.arange(V, dtype=f32), 0)
    add("constant", np.full(V, 1.25, f32), 0)
    add("all -inf", np.full(V, -np.inf, f32), 0)
    z = np.zeros(V, f32); z[1::2] = -0.0
    add("+0/-0 alternating", z, 0)
    z = np.zeros(V, f32); z[0::2] = -0.0
    add("-0/+0 alternating", z, 0)
    singles = sorted({i for i in SINGLE_IDS + (V - 3, V - 2, V - 1, 4 * (V // 4) - 1, 4 * (V // 4)) if 0 <= i < V})
    for i in singles:
        x = noise(); x[i] = 10.0
        add(f"one maximum at {i}", x, i)
    ties = [t for t in TIES if t[-1] < V]
    if V > 1:
        ties.append((0, V - 1))
    if V > 3:
        ties.append((0, 1, V - 1))
    if V % 4 and V > 8:     # one id in the last whole float4, one in the ids behind it
        ties += [(4 * (V // 4) - 2, V - 1), (2, 4 * (V // 4))]
    for t in ties:
        x = noise(); x[list(t)] = 10.0
        add(f"tie at {t}", x, t[0])
        x = -np.abs(noise()) - 1; x[list(t)] = 0.0; x[t[0]] = -0.0          # -0 first, +0 behind it, everything else negative: they are equal
        add(f"-0/+0 tie at {t}", x, t[0])
    p, q = V // 3, (2 * V) // 3
    x = noise(); x[q] = np.inf
    add("+inf once", x, q)
    if q > p:
        x = noise(); x[[p, q]] = np.inf
        add("+inf twice", x, p)
    x = np.full(V, -np.inf, f32); x[V - 1 - (V > 2)] = -2.5
    add("-inf but one", x, V - 1 - (V > 2))
    if V > 1:
        x = noise(); x[p] = FLT_MAX; x[p + 1] = np.inf
        add("FLT_MAX then +inf", x, p + 1)
        x = noise(); x[p] = np.inf; x[p + 1] = FLT_MAX
        add("+inf then FLT_MAX", x, p)
        x = np.zeros(V, f32); x[q] = DENORM
        add("denormal over zeros", x, q)
        x = np.full(V, -DENORM, f32); x[q] = -0.0
        add("-0 over negative denormals", x, q)
    # NaN rows
    add("all NaN", np.full(V, np.nan, f32), 0)
    x = noise(); x[0] = np.nan; x[V - 1] = 10.0
    add("NaN at 0", x, 0)
    x = np.full(V, np.nan, f32); x[V - 1] = 1.0
    add("NaN but the last", x, 0)
    if V > 1:
        x = np.full(V, np.nan, f32); x[0] = -np.inf
        add("-inf at 0, NaN behind", x, 0)
    for nan_at, max_at in ((4, 6), (4, 1028), (4, 2052), (1028, 1030), (1028, 2052), (1, 2), (1, V - 1), (16384, 16386), (1024, 2048), (V - 2, V - 1),
                           (9, 8), (1029, 5), (16392, 8), (7, 4), (V - 1, 0), (V - 1, V - 2)):   # (behind the maximum, in its thread)
        if 0 < nan_at < V and 0 <= max_at < V and nan_at != max_at:
            x = noise(); x[nan_at] = np.nan; x[max_at] = 10.0
            add(f"NaN at {nan_at}, maximum at {max_at}", x, max_at)
    if V > 8:
        m = V // 2
        x = noise(); x[[m - 1, m + 1]] = np.nan; x[m] = 10.0
        add("NaN on both sides of the maximum", x, m)
        x = noise(); x[1::2] = np.nan; x[0] = -3.5; x[(V - 1) & ~1] = 10.0     # every second element NaN: every float4 holds two
        add("every odd id NaN", x, (V - 1) & ~1)
        x = np.full(V, np.nan, f32); x[0] = -1.0; x[[m, m + 4]] = -1.0          # NaN everywhere but three equal values: id 0 stays
        add("NaN but three equal values", x, 0)
        x = np.full(V, np.nan, f32); x[0] = -1.0; x[m] = -0.5
        add("NaN but two values", x, m)
    return np.stack(rows), names, known


# ---- sampler ----------------------------------------------------------------------------------------------------------------------------------
SAMPLER_V = (1, 3, 63, 1023, 1025, 4097, 32001, 32767, 32768, 32769, 49999, 65535, 65536)
SAMPLER_K = (1, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65, 128, 1023, 1024)
DRAWS = (0, 1)
SEED = 2024


class Case:
    def __init__(self, name, logits, ring, topK, topP, temp, penalty):
        self.name, self.logits, self.ring = name, np.ascontiguousarray(logits, dtype=f32), [int(t) for t in ring]
        self.topK, self.topP, self.temp, self.penalty = int(topK), float(topP), float(temp), float(penalty)

    def args(self):
        return self.logits, self.ring, self.topK, self.topP, self.temp, self.penalty

    def __repr__(self):
        return f"{self.name} V={self.logits.size} K={self.topK} topP={self.topP} temp={self.temp} pen={self.penalty} ring={len(self.ring)}"


def grid_cases(V):
    """Every K of the list that fits (and K = V for V <= 1024) on N(0,1)*4 logits with a 64-entry ring drawn from [0, V + 50): some ids lie
    outside the vocabulary; the ring empties for a K of either kernel."""
    rng = np.random.default_rng(7 * V + 1)
    ks = sorted({k for k in SAMPLER_K if k <= V} | ({V} if V <= 1024 else set()))
    out = []
    for K in ks:
        lg = (rng.standard_normal(V) * 4).astype(f32)
        ring = rng.integers(0, V + 50, 64)
        ring[0] = V + int(rng.integers(0, 50))          # at least one id behind the vocabulary, and the vocabulary's last id
        ring[1] = V - 1
        out.append(Case("grid", lg, ring, K, 0.95 if K % 2 else 1.0, 0.8, 1.1))
    for K in sorted({k for k in (1, 17, 64, 65, 128) if k <= V} | {min(V, 40)}):
        out.append(Case("grid, empty ring", (rng.standard_normal(V) * 4).astype(f32), [], K, 0.95, 0.8, 1.1))
    return out


def _kth_largest_penalised(c):
    """The K-th largest value the sampler sorts (reference arithmetic, -0 folded into +0) and how many values are >= it."""
    l = c.logits
    v = l * (f32(1.0) / f32(c.temp))
    member = np.zeros(l.size, bool)
    r = np.asarray(c.ring, dtype=np.int64)
    member[r[r < l.size]] = True
    v = np.where(member, np.where(l < 0, v * f32(c.penalty), v / f32(c.penalty)), v).astype(f32) + f32(0.0)
    kth = np.sort(v)[::-1][c.topK - 1]
    return kth, int((v >= kth).sum())


def mass_tie_cases():
    """V = 32000, m ids at exactly 3.0 over N*2 - 10: the K-th place falls inside the tie.  The ring holds the lowest and the highest tied id, so
    those two are penalised out of the tie: m - 2 values stay equal, under the ten larger ones where those are planted.  Where more than 1024
    values are >= the K-th largest (asserted here on the reference's values: without the ten from m = 1027, with them from m = 1023), k_sample_small's
    survivor list overflows - its pivot never exceeds the K-th largest value - and the per-wave fallback runs.  1026 and 1027 are in the list so
    that the list's limit is straddled without the ten as well: 1024 survivors fit, 1025 do not."""
    V = 32000
    out = []
    for m in (1000, 1023, 1024, 1025, 1026, 1027, 1100, 5000):
        for top in (False, True):
            for K in (40, 64, 65, 200):
                rng = np.random.default_rng(m * 10 + K + top)
                lg = (rng.standard_normal(V) * 2 - 10).astype(f32)
                tied = np.sort(rng.choice(V, m, replace=False))
                lg[tied] = 3.0
                if top:
                    rest = np.setdiff1d(np.arange(V), tied)
                    lg[rng.choice(rest, 10, replace=False)] = 4.0 + np.arange(10, dtype=f32) * 0.25
                c = Case(f"mass tie m={m}{' under ten larger' if top else ''}", lg, [int(tied[0]), int(tied[-1])], K, 0.95, 0.8, 1.1)
                kth, n_ge = _kth_largest_penalised(c)
                assert n_ge == m - 2 + (10 if top else 0), (m, K, top, n_ge)
                assert (n_ge > 1024) == (m >= (1023 if top else 1027)), (m, K, top, n_ge)
                out.append(c)
    return out


def top_p_cases():
    """topP of 0, tiny, just under 1, 1 and above; and a topP < 1 that the fp32 running sum of all K probabilities never reaches (searched for, and
    asserted, on the reference's own probabilities: the cut then keeps all K and rescales by the sum it got to)."""
    V = 32000
    out = []
    for K in (40, 100):
        for topP in (0.0, 1e-30, 0.999999, 1.0, 1.5):
            rng = np.random.default_rng(K * 31 + int(topP * 1000))
            out.append(Case("topP", (rng.standard_normal(V) * 4).astype(f32), rng.integers(0, V, 64), K, topP, 0.8, 1.1))
        below_one = float(np.nextafter(f32(1.0), f32(0.0)))
        for seed in range(200):
            rng = np.random.default_rng(5000 + K * 200 + seed)
            c = Case("topP never reached", (rng.standard_normal(V) * 0.05).astype(f32), rng.integers(0, V, 64), K, below_one, 0.8, 1.1)
            _, _, probs = sampler_ref.sample(c.logits, c.ring, K, 1.0, c.temp, c.penalty, SEED, 0)     # no cut: the K probabilities as they are summed
            run = f32(0.0)
            for p in probs:
                run = f32(run + p)
            if run < f32(below_one):
                out.append(c)
                break
        else:
            raise AssertionError(f"no row found whose {K} probabilities sum below {below_one} in fp32")
    return out


def special_value_cases():
    """Zeros of both signs, the smallest denormals, both infinities and +-3e38 among ordinary logits, every one of them in the ring, under
    penalties below and above 1 and temperatures that overflow (1e-3 on 3e38) and underflow (1e3 on a denormal)."""
    out = []
    for V in (1025, 32768):
        for with_pinf in (False, True):
            for K in (40, 100):
                rng = np.random.default_rng(V + K + with_pinf)
                lg = (rng.standard_normal(V) * 4).astype(f32)
                special = [0.0, -0.0, DENORM, -DENORM, -np.inf, 3e38, -3e38] + ([np.inf] if with_pinf else [])
                at = rng.choice(V, 4 * len(special), replace=False)
                for j, i in enumerate(at):
                    lg[i] = special[j % len(special)]
                lg[rng.choice(np.setdiff1d(np.arange(V), at), 30, replace=False)] = 0.0      # more zeros than the ring holds: penalised and plain zeros tie
                ring = [int(i) for i in at] + [V - 1, V + 3]
                for temp, pen in ((0.8, 0.5), (1e-3, 1.1), (1e3, 1.1), (1.0, 1.0)):
                    out.append(Case(f"special values{' with +inf' if with_pinf else ''}", lg, ring, K, 0.95, temp, pen))
    return out


def sampler_groups():
    """-> {group name: [Case]}; one GPU test function per group keeps each at a few hundred one-shot calls."""
    g = {f"grid V={V}": grid_cases(V) for V in SAMPLER_V}
    mt = mass_tie_cases()
    g["mass ties K<=64"] = [c for c in mt if c.topK <= 64]
    g["mass ties K>64"] = [c for c in mt if c.topK > 64]
    g["topP"] = top_p_cases()
    g["special values"] = special_value_cases()
    return g


_GROUPS = None
_REF = {}


def groups():
    global _GROUPS
    if _GROUPS is None:
        _GROUPS = sampler_groups()
    return _GROUPS


GROUP_NAMES = tuple([f"grid V={V}" for V in SAMPLER_V] + ["mass ties K<=64", "mass ties K>64", "topP", "special values"])


def reference(group, i, draw):
    """sampler_ref.sample of case i of a group, computed once per session: (token, ids, probs)."""
    key = (group, i, draw)
    if key not in _REF:
        c = groups()[group][i]
        _REF[key] = sampler_ref.sample(*c.args(), SEED, draw)
    return _REF[key]


def ulps(a, b):
    """Largest |a - b| in units of the spacing at the larger magnitude (the measure of tests/test_gpu_sample.py); NaN against NaN counts 0, NaN
    against a number inf."""
    a = np.asarray(a, f32); b = np.asarray(b, f32)
    if a.shape != b.shape:
        return np.inf
    both_nan = np.isnan(a) & np.isnan(b)
    if np.any(np.isnan(a) != np.isnan(b)):
        return np.inf
    a = np.where(both_nan, f32(0), a); b = np.where(both_nan, f32(0), b)
    if a.size == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(f32)).astype(np.float64)
    return float(np.max(d))
