"""Session harness: scripts of calls on ONE long-lived object (a solo Context, a Batch or a DraftPair), held to fresh twins across re-captures.

Every other GPU test of the suite runs its call on a fresh object.  What they cannot see is a captured hipGraph that outlives something it holds: a
re-allocated scratch buffer, the sampler variant of the previous call, a ring that moved.  Nothing faults then and no single call is wrong - the ids
drift only in a process that did A, then B, then A again.  A script is such a process, written down (tests/session_cases.py), and this module runs it
against three oracles, all of them BYTE equalities of everything a step returns (no tolerance anywhere: the twins run the same kernels at the same
row counts, which tests/test_gpu_llama.py::test_results_are_bitwise_reproducible holds to reproduce):

  eager twin   the same steps on an object that lives under LLAMAHIP_NO_GRAPH=1: the variable is set around its creation AND around every one of its calls,
               because plan_create reads it, and a solo context makes its two plans lazily (llama_Eval's at the first Eval, the resident one at the first
               resident call), not in llama_NewContext.  It holds no captured address, so a stale graph shows at the first step that replays it; that it
               holds none is itself checked: at every step the long-lived object replays, the twin's own route trace must record the launches.
  fresh twin   a new object that runs only the ESSENTIAL steps.  It catches what graph and eager get wrong together: what a detour left behind.
  trace        on the long-lived object only: "a launch replayed from a captured graph records nothing" (include/llamahip.h, lh_route_trace), so a step
               declared `replay` must record no entry of its captured part and one declared `capture` / `eager` must record some.  Without this a
               script could pass by never replaying anything.

Two more things are done to the long-lived object alone.  The lh_ctx switches that choose a kernel (Step.env names that start with "lh:" - SWITCHES
below) are set on it and never on the twins, like the environment switches: the twins are the unswitched runs, so every step also holds switch-on bytes to
switch-off bytes.  And in front of EVERY step its context's weight images (the fp32 image of an f16 model's matrices, the int8 image of a block-int4
model's: one layer and the output matrix, shared by every plan of a size) are filled with 0xFF bytes (llamago_PoisonWeightImages): a launch that reads an
image slot which this call's own launches - or the replayed graph's own launches - did not fill computes from NaN / quant -1 and differs from both twins,
whatever ran before and however many layers the model has.

A step is `essential` (it changes what later results may depend on: cache rows below the final position, ring, draw counter, token history) or a
`detour` (by the API's contract its effects are gone when the next essential step runs).  The module needs no GPU: a backend is anything with
open() / setenv(); tests/test_session_cpu.py drives a toy backend and its mutants through the same run_script, tests/test_gpu_session.py the product.
"""
import re
from dataclasses import dataclass, field

import numpy as np

ESSENTIAL, DETOUR = "essential", "detour"
EAGER, CAPTURE, REPLAY = "eager", "capture", "replay"

# the entries of a route trace that name a kernel launch (the others - "feed_pass/..", "share_table/.." - are host decisions)
KERNEL_RE = r"^(k_|attention_gemm)"
# ... of a solo decode step: its attention launch (the decode GEMV launches record nothing); a prompt of >= 2 rows records /n<rows> instead
DECODE_RE = r"^k_attention[a-z_]*/[a-z]+\d+/n1$"
# ... of a pass over a row table (a lookup-draft verify pass of a solo context: the prompt Eval in front of a sampled loop has no row table)
ROWS_RE = r"^k_attention[a-z_]*/rows/"


@dataclass(frozen=True)
class Step:
    call: str                       # a method of the backend's session object
    args: dict = field(default_factory=dict)
    role: str = ESSENTIAL
    trace: str = None               # EAGER / CAPTURE / REPLAY, or None: the step launches nothing worth a statement (a setter, a read)
    fires: tuple = ()               # names of rows of session_cases.TRIGGERS this step fires
    graph_entries: str = KERNEL_RE  # which trace entries belong to the part of the call that runs from a captured graph
    env: tuple = ()                 # ((name, value or None), ...) set (unset) from this step on, around the long-lived object's calls only
    equals: int = None              # index of an earlier step whose result this one must repeat byte for byte
    twin: "Step" = None             # what the eager twin runs instead (same result keys), e.g. one long run as two shorter ones
    note: str = ""
    want: tuple = ()                # patterns of which each must match some entry of the long-lived object's route trace: the kernel family the step is there for
    wantnot: tuple = ()             # ... of which none may match any (tests/test_gpu_session.py asserts both; the toy has no kernel families)


@dataclass(frozen=True)
class Script:
    name: str
    kind: str                       # "solo" / "batch" / "pair" (a DraftPair: steps name their side, "target.Eval", "draft.Decode", or the pair's own calls)
    shape: str                      # key of mlapi.SHAPES
    ctx: int
    steps: tuple
    pods: int = 0
    doc: str = ""


class SessionMismatch(AssertionError):
    pass


def first_difference(a, b):
    """None when the two results (dicts of arrays) are byte-equal, else a sentence naming the first differing element."""
    if sorted(a) != sorted(b):
        return f"result keys differ: {sorted(a)} against {sorted(b)}"
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape:
            return f"{k}: {x.dtype}{x.shape} against {y.dtype}{y.shape}"
        if x.tobytes() == y.tobytes():
            continue
        xb = np.frombuffer(x.tobytes(), dtype=np.uint8).reshape(-1, x.dtype.itemsize)
        yb = np.frombuffer(y.tobytes(), dtype=np.uint8).reshape(-1, x.dtype.itemsize)
        i = int(np.flatnonzero((xb != yb).any(axis=1))[0])
        idx = tuple(int(v) for v in np.unravel_index(i, x.shape)) if x.shape else ()
        return f"{k}{list(idx)}: {x.reshape(-1)[i]!r} against {y.reshape(-1)[i]!r} ({int((xb != yb).any(axis=1).sum())} of {xb.shape[0]} elements differ)"
    return None


def classify(trace, pattern):
    """The trace entries of a step's captured part."""
    rx = re.compile(pattern)
    return [e for e in trace if rx.search(e)]


ORACLES = ("trace", "eager", "fresh", "repeat")


def run_script(script, backend, weights, report=None, trace_strict=True, ask=ORACLES):
    """Runs `script` on three objects of `backend` and raises SessionMismatch at the first step an oracle refuses.  report (a list) receives one
    line per step: index, call, role, the declared and the observed trace class - the evidence that each trigger fired and was replayed.
    ask: the oracles that may refuse, asked in the order of ORACLES (all of them, except where tests/test_session_cpu.py shows what ONE oracle says of a
    mutant that an earlier one reports first; the twins run every step either way).  Returns the long-lived object's route trace of every step."""
    objs, traces = {}, []
    try:
        objs["long"] = backend.open(script, weights, eager=False, role="long")
        objs["eager"] = backend.open(script, weights, eager=True, role="eager")
        objs["fresh"] = backend.open(script, weights, eager=False, role="fresh")
        results, switched = [], {}
        for i, st in enumerate(script.steps):
            where = f"script {script.name} [{weights}] step {i} ({st.call} {_brief(st.args)})"
            switched.update(st.env)
            for name, value in switched.items():   # the switches hold for the long-lived object alone: the twins run unswitched
                backend.setenv(name, value)
            try:
                got, trace = objs["long"].call(st, traced=True)
            finally:
                for name in switched:
                    backend.setenv(name, None)
            results.append(got)
            traces.append(trace)
            entries = classify(trace, st.graph_entries)
            if report is not None:
                report.append(f"{script.name}[{weights}] {i:2d} {st.call:<18} {st.role:<9} declared {st.trace or '-':<7} observed "
                              f"{'replay' if not entries else 'launch'} ({len(entries)} of {len(trace)} entries{': ' + entries[0] if entries else ''})"
                              f"{' fires ' + ','.join(st.fires) if st.fires else ''}")
            bad = None
            if st.trace == REPLAY and entries:
                bad = f"{where}: oracle trace: declared replay, but the call launched {len(entries)} kernels outside a graph, first {entries[0]}"
            if st.trace in (EAGER, CAPTURE) and not entries:
                bad = (f"{where}: oracle trace: declared {st.trace}, but the route trace holds no entry of the captured part "
                       f"(the whole call replayed: the trigger in front of it did not fire)")
            if bad and trace_strict and "trace" in ask:
                raise SessionMismatch(bad)
            if bad and report is not None:
                report.append("  TRACE MISMATCH " + bad)
            twin, twin_trace = objs["eager"].call(st.twin or st, traced=True)
            if "eager" in ask and st.trace == REPLAY and not classify(twin_trace, st.graph_entries):
                raise SessionMismatch(f"{where}: oracle eager twin: the twin itself recorded no launch of the captured part - it replays a graph of its own "
                                      f"and would repeat a stale one byte for byte (was it created, and were its plans made, under LLAMAHIP_NO_GRAPH=1?)")
            d = first_difference(got, twin)
            if d and "eager" in ask:
                raise SessionMismatch(f"{where}: oracle eager twin: {d}")
            if st.role == ESSENTIAL:
                fresh, _ = objs["fresh"].call(st, traced=False)
                d = first_difference(got, fresh)
                if d and "fresh" in ask:
                    raise SessionMismatch(f"{where}: oracle fresh twin: {d}")
            if st.equals is not None:
                d = first_difference(got, results[st.equals])
                if d and "repeat" in ask:
                    raise SessionMismatch(f"{where}: oracle repeat of step {st.equals}: {d}")
    finally:
        for o in objs.values():
            o.close()
        backend.restore_env()
    return traces


def _brief(args):
    out = []
    for k, v in args.items():
        s = repr(v)
        out.append(f"{k}={s if len(s) <= 24 else s[:21] + '...'}")
    return ", ".join(out)


# ---- deterministic token material (scripts are static: no step depends on an id an earlier step produced) ---------------------------------------------
def toks(n, seed, vocab):
    """n token ids in [1, vocab) from a fixed LCG: the same list on every machine."""
    out, s = [], (seed * 2654435761 + 12345) & 0xFFFFFFFF
    for _ in range(n):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        out.append(1 + (s >> 8) % (vocab - 1))
    return out


def swap_positions(past, n_steps, ctx, keep):
    """The position behind n_steps resident decode steps that start at `past`, with the reference's context swap (server.go:160-172) whenever the
    window is full: the run of (past - keep) / 2 tokens is re-fed at position keep."""
    for _ in range(n_steps):
        if past >= ctx:
            past = keep + (past - keep) // 2
        past += 1
    return past


# ---- the product behind the harness (imports nothing of the package until a session is opened) --------------------------------------------------------
def _u32(x):
    return np.asarray(x, dtype=np.uint32)


def _stats(st):
    return _u32([[s[k] for k in ("passes", "rows", "drafted", "accepted", "empty")] for s in (st if isinstance(st, list) else [st])])


def _pairs(tr):
    return _u32([list(p) for p in tr]).reshape(-1, 2)


class EnvPatch:
    """pytest's monkeypatch, as far as ProductBackend uses it, for a process without pytest."""

    def __init__(self):
        self.saved = {}

    def setenv(self, name, value):
        import os
        self.saved.setdefault(name, os.environ.get(name))
        os.environ[name] = value

    def delenv(self, name, raising=False):
        import os
        self.saved.setdefault(name, os.environ.get(name))
        os.environ.pop(name, None)

    def undo(self):
        import os
        for name, value in self.saved.items():
            os.environ.pop(name, None) if value is None else os.environ.__setitem__(name, value)
        self.saved = {}


# the lh_ctx switches a Step.env entry may name ("1" on, None / "0" off) -> the setter of mlapi.Context / mlapi.Batch
SWITCHES = {"lh:f16_stream": "SetF16Stream", "lh:q4_stream": "SetQ4Stream", "lh:f16_tiles": "SetF16Tiles"}
WIDE = ("f16", "q4")   # the weight types whose plans read a context-owned image (Plan::md_wide)
# the pairs of a "pair" script, by the target's weight type: (draft's weight type, draft's seed, the seed of ReplaceDraft's model).  The f16 draft has the
# target's SHAPE and another seed: both plans then share one image on the pair's lh_ctx (wide_image keys by size), two models' matrices pass through it
PAIRS = {"f32": ("q8", 4321, 777), "f16": ("f16", 4321, 777), "q4": ("f32", 4321, 777)}
MODEL_SEED = 1234


class ProductBackend:
    """models(shape, weights, seed=MODEL_SEED) -> an mlapi.Model (kept by the caller); monkeypatch: pytest's, for the environment switches."""

    def __init__(self, models, monkeypatch):
        self.models, self.mp = models, monkeypatch
        self.switches = {}

    def setenv(self, name, value):
        if name in SWITCHES:
            self.switches[name] = value == "1"
        elif value is None:
            self.mp.delenv(name, raising=False)
        else:
            self.mp.setenv(name, value)

    def restore_env(self):
        self.switches = {}
        self.mp.undo()

    def open(self, script, weights, eager, role="long"):
        model = self.models(script.shape, weights)
        wide = weights in WIDE
        if script.kind == "pair":
            dw, dseed, rseed = PAIRS[weights]
            draft, repl = self.models(script.shape, dw, dseed), self.models(script.shape, dw, rseed)
            wide = wide or dw in WIDE
            make = lambda: _PairSession(model, draft, repl, script.ctx)   # noqa: E731
        elif script.kind == "solo":
            make = lambda: _SoloSession(model, script.ctx)   # noqa: E731
        else:
            make = lambda: _BatchSession(model, script.ctx, script.pods)   # noqa: E731
        obj = _under_no_graph(self.mp, eager, make)
        obj.mp, obj.eager, obj.backend, obj.long, obj.wide = self.mp, eager, self, role == "long", wide
        return obj


def _under_no_graph(mp, eager, fn):
    """fn() with LLAMAHIP_NO_GRAPH=1 set (eager) - every plan made inside is eager for life - or surely unset (the other objects)."""
    mp.delenv("LLAMAHIP_NO_GRAPH", raising=False)
    if eager:
        mp.setenv("LLAMAHIP_NO_GRAPH", "1")
    try:
        return fn()
    finally:
        mp.delenv("LLAMAHIP_NO_GRAPH", raising=False)


class _Session:
    mp, eager, backend, long, wide, has_plan = None, False, None, False, False, False

    def _front(self):
        """What only the long-lived object gets in front of a step: the lh_ctx switches as the script has them now (a setter that repeats the value changes
        nothing), then the poison.  The images exist from the first plan on (wide_image in plan_create; a solo context and the contexts of a pair make their
        plans lazily): from then on the fill must report bytes for an f16 / block-int4 context, and it must never report any for an fp32 / block-int8 one."""
        if not self.long:
            return
        dev = self.device_object()
        for name, setter in SWITCHES.items():
            if hasattr(dev, setter):
                getattr(dev, setter)(self.backend.switches.get(name, False))
        n = dev.PoisonWeightImages()
        if self.wide:
            assert (n > 0) == self.has_plan, f"PoisonWeightImages filled {n} bytes on an f16 / block-int4 context {'with' if self.has_plan else 'without'} plans"
        else:
            assert n == 0, f"PoisonWeightImages filled {n} bytes on a context of fp32 / block-int8 plans"

    def call(self, st, traced):
        """Every call of the eager twin runs under LLAMAHIP_NO_GRAPH=1: plans, and the contexts a step opens, are made lazily inside calls."""
        from llama_go_amd.mlapi import route_trace
        self._front()
        side, _, name = st.call.rpartition(".")
        fn = getattr(getattr(self, side) if side else self, name)
        if name not in ("SetKeepCount", "CacheImage"):
            self.has_plan = True
        if traced:
            return _under_no_graph(self.mp, self.eager, lambda: route_trace(lambda: fn(**st.args)))
        return _under_no_graph(self.mp, self.eager, lambda: fn(**st.args)), []


class _SoloSession(_Session):
    def __init__(self, model, ctx, context=None):
        """context: a Context that belongs to someone else (a side of a DraftPair), not freed here."""
        self.model, self.ctx = model, ctx
        self.c, self.owned = model.NewContext(ctx) if context is None else context, context is None
        self.others = {}

    def device_object(self):
        return self.c

    def close(self):
        for o in self.others.values():
            o.free()
        self.others = {}
        if self.owned:
            self.c.free()

    # every method returns a dict of arrays: everything the call hands back
    def Eval(self, tokens, past):
        return {"logits": self.c.Eval(tokens, past)}

    def GreedyDecode(self, prompt, n):
        ids, lg = self.c.GreedyDecode(prompt, n)
        return {"ids": _u32(ids), "logits": lg}

    def Decode(self, first, past, n):
        """The resident greedy loop continuing from (first, past): llamago_DecodeGreedyResident."""
        from llama_go_amd.mlapi import decode_greedy_resident
        ids, lg = decode_greedy_resident(self.c, first, past, n, want_logits=True)
        return {"ids": _u32(ids), "logits": lg}

    def DecodeSplit(self, first, past, counts, keep):
        """Decode in len(counts) calls, each continuing where the one before stopped (its last id is the next one's first token)."""
        ids, res = [], None
        for n in counts:
            res = self.Decode(first, past, n)
            ids += [int(t) for t in res["ids"]]
            past, first = swap_positions(past, n, self.ctx, keep), ids[-1]
        return {"ids": _u32(ids), "logits": res["logits"]}

    def SampleDecode(self, prompt, n, topK, seed):
        return {"ids": _u32(self.c.SampleDecode(prompt, n, topK=topK, seed=seed))}

    def Score(self, tokens, past):
        return {"rows": self.c.Score(tokens, past)}

    def Verify(self, tokens, past):
        ids, a, lg = self.c.Verify(tokens, past, want_logits=True)
        return {"ids": _u32(ids), "accepted": _u32([a]), "logits": lg}

    def DecodeLookup(self, first, past, n, draft_max, ngram_max=3, ngram_min=1, corpus=None):
        ids, lg, st, tr = self.c.DecodeLookup(first, past, n, draft_max, ngram_max, ngram_min, corpus=corpus, want_logits=True)
        return {"ids": _u32(ids), "logits": lg, "stats": _stats(st), "passes": _pairs(tr)}

    def SampleDecodeLookup(self, prompt, n, draft_max, ring, topK, seed, ngram_max=3, ngram_min=1):
        ids, st, tr = self.c.SampleDecodeLookup(prompt, n, draft_max, ngram_max, ngram_min, ring_size=ring, topK=topK, seed=seed)
        return {"ids": _u32(ids), "stats": _stats(st), "passes": _pairs(tr)}

    def EmbeddingEval(self, tokens, past):
        """Embedding output switched on (the host mirror has no switch back: it stays on for the rest of the script, the fresh twin never has it), one Eval."""
        self.c.EnableEmbedding()
        return {"logits": self.c.Eval(tokens, past), "embedding": self.c.Embedding()}

    def SetKeepCount(self, keep):
        self.c.SetKeepCount(keep)
        return {}

    def CacheImage(self, pos):
        """K and V rows [0, pos) of every layer."""
        hp = self.model.hp
        d, L = hp.embdSize, hp.layersCount
        return {("k", "v")[w]: np.stack([self.c.CacheRead(w, l * self.ctx * d, pos * d) for l in range(L)]) for w in (0, 1)}

    def OpenOther(self, ctx, tokens, past):
        o = self.others["o"] = self.model.NewContext(ctx)
        return {"logits": o.Eval(tokens, past)}

    def CloseOther(self):
        self.others.pop("o").free()
        return {}


class _BatchSession(_Session):
    def __init__(self, model, ctx, pods):
        from llama_go_amd.mlapi import Batch
        self.model, self.ctx, self.pods = model, ctx, pods
        self.b = Batch(model, ctx, pods)
        self.sampling = False
        self.has_plan = True   # (a batch makes its pods' plans when it is made)

    def device_object(self):
        return self.b

    def close(self):
        self.b.free()

    def Prompt(self, prompts):
        self.sampling = False   # (llamago_BatchPrompt clears the sampler)
        return {"ids": _u32(self.b.Prompt(prompts))}

    def Tick(self):
        res = {"ids": _u32(self.b.Tick())}
        if self.sampling:   # rings, ring positions and draw counters behind EVERY sampled tick: a difference is reported at the tick that made it
            res.update(self.SamplerState())
        return res

    def Set(self, tokens, past):
        self.b.Set(tokens, past)
        return {}

    def Decode(self, first, past, n):
        ids, lg = self.b.Decode(first, past, n, want_logits=True)
        return {"ids": _u32(ids), "logits": lg}

    def _fed(self, res):
        ids, last = res
        return {"ids": _u32([0xFFFFFFFF if t is None else t for t in ids]), "last": last}

    def Feed(self, tokens, past):
        return self._fed(self.b.Feed(tokens, past, want_logits=True))

    def FeedSample(self, tokens, past, flags=None):
        return self._fed(self.b.FeedSample(tokens, past, flags, want_logits=True))

    def SetSampler(self, topK, seed, ring):
        self.b.SetSampler(topK=topK, seed=seed, ringSize=ring)
        self.sampling = True
        return self.SamplerState()

    def ClearSampler(self):
        self.b.ClearSampler()
        self.sampling = False
        return {}

    def SamplerState(self):
        st = [self.b.SamplerState(p) for p in range(self.pods)]
        return {"rings": _u32([s[0] for s in st]), "ring_pos": _u32([s[1] for s in st]), "draws": np.asarray([s[2] for s in st], dtype=np.uint64)}

    def Fork(self, src, dst, n_pos):
        self.b.Fork(src, dst, n_pos)
        g, ln = self.b.ShareInfo()
        return {"group": _u32(g), "length": _u32(ln)}

    def _lookup(self, res):
        ids, lg, st, tr = res
        n = max(len(t) for t in tr) if tr else 0
        passes = np.full((self.pods, max(n, 1), 2), 0xFFFFFFFF, dtype=np.uint32)
        for p, t in enumerate(tr):
            if t:
                passes[p, :len(t)] = _pairs(t)
        return {"ids": _u32(ids), "logits": lg, "stats": _stats(st), "passes": passes}

    def DecodeLookup(self, first, past, n, draft_max, ngram_max=3, ngram_min=1):
        return self._lookup(self.b.DecodeLookup(first, past, n, draft_max, ngram_max, ngram_min, want_logits=True))

    def DecodeSampleLookup(self, first, past, n, draft_max, ngram_max=3, ngram_min=1):
        res = self._lookup(self.b.DecodeSampleLookup(first, past, n, draft_max, ngram_max, ngram_min, want_logits=True))
        res.update(self.SamplerState())
        return res

    def CacheImage(self, pos):
        """K and V rows [0, pos[p]) of every layer of every pod, one after the other."""
        hp = self.model.hp
        d, L = hp.embdSize, hp.layersCount
        return {("k", "v")[w]: np.concatenate([self.b.CacheRead(p, w, l * self.ctx * d, pos[p] * d) for p in range(self.pods) for l in range(L)])
                for w in (0, 1)}

    def OtherBatch(self, pods, prompts, ticks):
        """A second batch on the same model created, ticked and freed."""
        from llama_go_amd.mlapi import Batch
        o = Batch(self.model, self.ctx, pods)
        try:
            ids = [o.Prompt(prompts)] + [o.Tick() for _ in range(ticks)]
            return {"ids": _u32(ids)}
        finally:
            o.free()


class _PairSession(_Session):
    """A DraftPair: .target and .draft are solo sessions over the pair's two contexts (a step names its side: "target.Eval", "draft.Decode"); the pair's own
    calls are DecodeDraft, ReplaceDraft and a CacheImage of both sides."""

    def __init__(self, target_model, draft_model, replacement_model, ctx):
        from llama_go_amd.mlapi import DraftPair
        self.ctx, self.replacement = ctx, replacement_model
        self.pair = DraftPair(target_model, draft_model, ctx)
        self.target = _SoloSession(target_model, ctx, self.pair.target)
        self.draft = _SoloSession(draft_model, ctx, self.pair.draft)

    def device_object(self):
        return self.pair.target   # (both sides evaluate in the pair's one lh_ctx: its switches, its images)

    def close(self):
        self.pair.free()

    def DecodeDraft(self, first, past, n, draft_len):
        ids, lg, st, tr = self.pair.DecodeDraft(first, past, n, draft_len, want_logits=True)
        return {"ids": _u32(ids), "logits": lg, "stats": _stats(st), "passes": _pairs(tr)}

    def ReplaceDraft(self):
        """The draft context freed beside the target's live graphs, a fresh one over another model of the draft's shape and type in its place."""
        self.draft = _SoloSession(self.replacement, self.ctx, self.pair.ReplaceDraft(self.replacement))
        return {}

    def CacheImage(self, pos, draft_pos):
        t, d = self.target.CacheImage(pos), self.draft.CacheImage(draft_pos)
        return {"k": t["k"], "v": t["v"], "draft_k": d["k"], "draft_v": d["v"]}
