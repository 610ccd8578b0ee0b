"""A pure-Python toy backend for the session harness (tests/session_ref.py): the calls the scripts use, over a model that is a hash of (token history,
position), with the capture logic of csrc/plan.hip in miniature - buffers with an identity, graphs that remember the buffers they were captured on, the
staleness keys, the eager first pass.  A freed buffer poisons what is read from it, so a graph that outlives one of its buffers computes garbage, as a real
one may.  tests/test_session_cpu.py runs every script on the clean toy (all three oracles must hold) and on mutants of it (each must be reported).

Mutants (ToyBackend(mutant=...)):
  growth_keeps_graph   plan_ensure_rows re-allocates the scratch and forgets drop_graphs
  partial_invalidation ensure_out_tokens drops the one-step greedy slot only, not the multi-step one
  variant_kept         a topK flip across 64 keeps the captured sampler variant
  ring_not_reinit      a second SetSampler with a smaller ring leaves the ring's old content
  detour_leaves_row    a Score at position P also overwrites cache row P - 1
  draw_not_restored    SampleDecode does not restart the draw counter
  twin_not_eager       (a mutant of the harness's footing, not of the product) the object opened as the eager twin captures graphs like any other
  switch_not_in_key    the stream switch is no field of the lookup pass's key (and nothing clears its warm bits): a toggle replays the graph of the other value.  The bytes are
                       equal by design - both values compute the same - so only the TRACE oracle can report it
  warm_not_cleared     a switch change re-keys the tick but leaves its warm bit: the kernel the new value chooses has its first launch inside a capture, without the attribute
                       an eager launch sets (Dev.lds), and the graph computes garbage
  image_site_unfilled  under the stream switch the multi-row launch site reads its image slot without filling it: right bytes as long as an earlier call left the right
                       matrix there (the toy WITHOUT poison passes), garbage once the image is poisoned between steps
  draft_leaves_smp     a draft run does not reset Spec::smp: behind a sampled lookup run it samples
  replace_frees_out    ReplaceDraft frees the TARGET's output list with the draft's and gives the plan a new one, dropping no graph: the resident graph writes into the freed list

The device in miniature (Dev) is what one lh_ctx owns: the stream switch with its generation counter, the grow-only split-K buffer, the kernel attributes set by eager launches,
and the weight image - one slot per launch site, filled by a call in front of its read (with the matrix of the plan's model: the two plans of a pair share the slots) and
poisoned in front of every step of the long-lived object.
"""
import numpy as np

M64 = (1 << 64) - 1
POISON = 0x5A5A5A5A5A5A5A5A
VOCAB = 509
GRAPH_MULTI = 8
FEED_PASS_ROWS, FEED_SOLO_MIN = 64, 129


def mix(*xs):
    z = 0x9E3779B97F4A7C15
    for x in xs:
        z = ((z ^ (int(x) & M64)) * 0xBF58476D1CE4E5B9) & M64
        z ^= z >> 29
    return z


def greedy(c):
    return mix(c, 99) % VOCAB


def logits(c):
    return np.array([mix(c, j) for j in range(8)], dtype=np.uint64)


class Buf:
    """Device memory with an identity: free() poisons every later read."""

    def __init__(self, n):
        self.d, self.freed = [0] * n, False

    def r(self, i):
        return self.d[i] ^ POISON if self.freed else self.d[i]

    def w(self, i, v):
        self.d[i] = v

    def free(self):
        self.freed = True


IMAGE_SITES = ("rows",)   # the multi-row launch sites that read the image (Plan.eval of >= 2 rows, a feed pass, a pods x R pass)


class Dev:
    """What an lh_ctx owns (see the module's docstring).  own: the Step.env name of the stream switch of the plans' weight type, or None (fp32, block-int8: key 0)."""

    def __init__(self, be, weights, poison):
        self.be, self.poison = be, poison
        self.own = {"f16": "lh:f16_stream", "q4": "lh:q4_stream"}.get(weights)
        self.sw, self.gen = False, 0
        self.image, self.lds = {}, set()
        self.splitk_cap, self.splitk_gen = 0, 0

    def begin_call(self):
        """lh_ctx_set_*_stream as the harness has it now (a change counts), then the poison"""
        v = self.own is not None and self.be.env.get(self.own) == "1"
        if v != self.sw:
            self.sw, self.gen = v, self.gen + 1
        if self.poison:
            self.image.clear()

    def stream_key(self):
        return (self.gen << 1) | int(self.sw) if self.own else 0

    def variant(self):
        return "h" if self.sw else "w"

    def ensure_splitk(self, n):
        if n > self.splitk_cap:
            self.splitk_cap, self.splitk_gen = n, self.splitk_gen + 1

    def weights(self, site, model):
        """The launch site's matrix: 0 when it reads the right one, garbage otherwise.  Under the switch the site reads the model's own halves / nibbles; without it the
        call fills the slot in front of the read."""
        if self.sw:
            if self.be.mutant != "image_site_unfilled":
                return 0
        else:
            self.image[site] = model
        return 0 if self.image.get(site) == model else mix(POISON, 5)


class Cache:
    def __init__(self, ctx):
        self.ctx, self.rows, self.hist = ctx, [0] * ctx, [None] * ctx

    def write(self, pos, tok):
        self.rows[pos], self.hist[pos] = mix(tok, pos + 1), tok

    def chain(self, pos):
        c = 0
        for p in range(pos + 1):
            c = mix(c, self.rows[p])
        return c


class Plan:
    """One plan over a cache: scratch for n_cap rows, the decode graphs, the sampler and lookup state of the resident calls."""
    STEP, ADV1, ADVN, SMP1, SMPN = range(5)

    def __init__(self, be, cache, eager, trace, dev, model="M"):
        self.be, self.cache, self.use_graph, self.trace, self.dev, self.model = be, cache, not eager, trace, dev, model
        self.n_cap, self.scratch, self.scratch_gen = 0, None, 0
        self.graphs = {}
        self.sp = {"token": 0, "past": 0, "step": 0}
        self.out, self.out_cap = None, 0
        self.ring, self.ring_cap, self.smp_topk = None, 0, 0
        self.ss = {"topK": 0, "seed": 0, "draw": 0, "ring_size": 1, "ring_pos": 0}
        self.score_cap, self.keep = 0, 0
        self.spec_warm, self.spec_graph, self.spec_corpus, self.spec_seen, self.spec_smp = set(), None, None, 0, False
        self.ensure_rows(1)

    def drop(self, slots):
        for s in slots:
            self.graphs.pop(s, None)

    def ensure_rows(self, n):
        if n <= self.n_cap:
            return
        if self.scratch:
            self.scratch.free()
        self.scratch, self.n_cap = Buf(n), n
        self.scratch_gen += 1
        if self.be.mutant != "growth_keeps_graph":
            self.drop(range(5))

    def ensure_out(self, n):
        if n <= self.out_cap:
            return
        if self.out:
            self.out.free()
        self.out_cap = max(n, 4096)
        self.out = Buf(self.out_cap)
        self.drop([Plan.ADV1] if self.be.mutant == "partial_invalidation" else [Plan.ADV1, Plan.ADVN, Plan.SMP1, Plan.SMPN])

    # ---- kernels: they work on the buffers they are handed, which a graph fixes at capture ----
    def k_rows(self, scratch, tokens, past, w=0):
        for i, t in enumerate(tokens):
            self.cache.write(past + i, t)
            scratch.w(i, self.cache.chain(past + i) ^ w)

    def k_decode(self, scratch, out, ring, variant, adv):
        sp = self.sp
        self.cache.write(sp["past"], sp["token"])
        scratch.w(0, self.cache.chain(sp["past"]))
        if adv:
            tok = greedy(scratch.r(0)) if adv == 1 else sample(scratch.r(0), self.ss, ring, 0, variant)
            out.w(sp["step"], tok)
            sp["token"], sp["past"], sp["step"] = tok, sp["past"] + 1, sp["step"] + 1

    def variant(self):
        return "small" if self.smp_topk <= 64 else "large"

    def decode_steps(self, n, sampled):
        """n resident steps: multi-step graph launches as far as they fit, single steps for the rest (launch_resident_steps)."""
        adv = 2 if sampled else 1
        slot1, slotn = (Plan.SMP1, Plan.SMPN) if sampled else (Plan.ADV1, Plan.ADVN)
        if not self.use_graph:
            for _ in range(n):
                self.trace.append("k_attention/hd64/n1")
                self.k_decode(self.scratch, self.out, self.ring, self.variant(), adv)
            return
        self.graph(slotn, GRAPH_MULTI)
        done = 0
        while done + GRAPH_MULTI <= n:
            self.launch(slotn, GRAPH_MULTI, adv)
            done += GRAPH_MULTI
        if done < n:
            self.graph(slot1, 1)
            for _ in range(n - done):
                self.launch(slot1, 1, adv)

    def graph(self, slot, reps):
        if slot not in self.graphs:
            self.trace.extend(["k_attention/hd64/n1"] * reps)
            self.graphs[slot] = (self.scratch, self.out, self.ring, self.variant())

    def launch(self, slot, reps, adv):
        for _ in range(reps):
            self.k_decode(*self.graphs[slot], adv)

    def eval(self, tokens, past):
        """llama.Eval on this plan: one token through the G_STEP graph, more as an eager pass."""
        n = len(tokens)
        if n == 1 and self.use_graph:
            self.graph(Plan.STEP, 1)
            self.sp.update(token=tokens[0], past=past, step=0)
            self.launch(Plan.STEP, 1, 0)
            return
        self.ensure_rows(n)
        if n >= 89:
            self.dev.ensure_splitk(n)   # (the tile GEMMs' split-K buffer / planes, the context's: grow-only)
        self.trace.append(f"k_attention/hd64/n{n}")
        self.k_rows(self.scratch, tokens, past, self.dev.weights("rows", self.model) if n >= 2 else 0)

    def resident(self, first, past, n, sampled, step0):
        """resident_steps_swapping: the steps, with the reference's context swap whenever the window is full."""
        self.sp.update(token=first, past=past, step=step0)
        done, ctx = 0, self.cache.ctx
        while done < n:
            if self.sp["past"] >= ctx:
                p, pending = self.sp["past"], self.sp["token"]
                m = (p - self.keep) // 2
                refeed = [self.cache.hist[p - (m - 1) + i] for i in range(m - 1)] + [pending]
                if m:
                    self.eval(refeed, self.keep) if len(refeed) > 1 else self.k_rows(self.scratch, refeed, self.keep)
                self.sp["past"] = self.keep + m
            k = min(n - done, ctx - self.sp["past"])
            self.decode_steps(k, sampled)
            done += k

    def arm_sampler(self, prompt, ring_size, topK, seed):
        """The front of decode_sample: variant, ring, sampler state."""
        if (topK <= 64) != (self.smp_topk <= 64) and self.be.mutant != "variant_kept":
            self.drop([Plan.SMP1, Plan.SMPN])
        self.smp_topk = topK
        if ring_size > self.ring_cap:
            if self.ring:
                self.ring.free()
            self.ring, self.ring_cap = Buf(ring_size), ring_size
            self.drop([Plan.SMP1, Plan.SMPN])
        for i in range(ring_size):
            self.ring.w(i, 0)
        for i, t in enumerate(prompt):
            self.ring.w(i % ring_size, t)
        draw = self.ss["draw"] if self.be.mutant == "draw_not_restored" else 0
        self.ss.update(topK=topK, seed=seed, draw=draw, ring_size=ring_size, ring_pos=len(prompt))

    # ---- lookup-draft passes (spec_pass): eager the first time at a row count, then a graph behind a staleness key ----
    def spec_pass(self, R, lp, smp, out_off, left):
        corpus = self.spec_corpus
        keyed = self.be.mutant != "switch_not_in_key"
        now = self.dev.stream_key() if keyed else 0
        key = (R, lp, id(corpus), id(self.out), out_off, self.scratch_gen, self.dev.splitk_gen, smp, smp and self.smp_topk <= 64, id(self.ring) if smp else 0, now)
        if self.spec_seen != now:   # f16_stream_sync: the kernels the new value chooses have their first launch in an eager pass
            self.spec_warm.clear()
            self.spec_seen = now
        bufs = (self.scratch, self.out, self.ring, self.variant())
        if not self.use_graph or R not in self.spec_warm:
            self.spec_warm.add(R)
            self.trace.append(f"k_attention/rows/hd64/n{R}")
        else:
            if self.spec_graph and self.spec_graph[0] != key:
                self.spec_graph = None
            if not self.spec_graph:
                self.trace.append(f"k_attention/rows/hd64/n{R}")
                self.spec_graph = (key, bufs)
            bufs = self.spec_graph[1]
        return self.k_spec(*bufs, R, smp, out_off, left)

    def k_spec(self, scratch, out, ring, variant, R, smp, out_off, left, draft=None):
        """One pass: the pending token and the accepted part of a draft of R - 1, one id each; the rejected rows stay behind in the cache above the position.
        draft: the cache of a draft model, whose state decides how much is accepted and which follows the accepted tokens."""
        sp = self.sp
        m = min(1 + mix(self.cache.chain(max(sp["past"] - 1, 0)), R, *([draft.chain(max(sp["past"] - 1, 0))] if draft else [])) % R, left)
        for i in range(m):
            self.cache.write(sp["past"], sp["token"])
            scratch.w(i, self.cache.chain(sp["past"]))
            tok = sample(scratch.r(i), self.ss, ring, 0, variant) if smp else greedy(scratch.r(i))
            out.w(out_off + sp["step"], tok)
            if draft:
                draft.write(sp["past"], sp["token"])
            sp["token"], sp["past"], sp["step"] = tok, sp["past"] + 1, sp["step"] + 1
        for i in range(m, R):
            if sp["past"] + i - m < self.cache.ctx:
                self.cache.rows[sp["past"] + i - m] = mix(7, i)
        return m

    def lookup(self, first, past, n, draft_max, ngram_max, ngram_min, corpus, smp, out_off):
        R = draft_max + 1
        self.ensure_rows(R)
        self.ensure_out(n + out_off)
        if corpus is not None and (self.spec_corpus is None or len(corpus) > len(self.spec_corpus.d)):
            self.spec_corpus = Buf(len(corpus))
        self.sp.update(token=first, past=past, step=0)
        self.spec_smp = smp
        passes = []
        while self.sp["step"] < n:
            m = self.spec_pass(R, (draft_max, ngram_max, ngram_min, len(corpus or ())), smp, out_off, n - self.sp["step"])
            passes.append((R - 1, m - 1))
        ids = [self.out.r(out_off + i) for i in range(n)]
        st = [len(passes), R, sum(p[0] for p in passes), sum(p[1] for p in passes), 0]
        return ids, st, passes


def sample(c, ss, ring, base, variant):
    k = ss["topK"] if variant == "large" else min(ss["topK"], 64)
    rh = mix(*[ring.r(base + i) for i in range(ss["ring_size"])])
    tok = mix(c, rh, ss["draw"], ss["seed"], k) % VOCAB
    ring.w(base + ss["ring_pos"] % ss["ring_size"], tok)
    ss["draw"], ss["ring_pos"] = ss["draw"] + 1, ss["ring_pos"] + 1
    return tok


def _u32(x):
    return np.asarray(x, dtype=np.uint32)


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


class ToySolo:
    """A context: one cache, the plan llama_Eval runs on and the plan of the resident calls."""

    def __init__(self, be, ctx, eager, dev, model="M", trace=None):
        self.be, self.ctx, self.eager, self.dev, self.trace = be, ctx, eager, dev, [] if trace is None else trace
        self.cache = Cache(ctx)
        self.ml, self.res = Plan(be, self.cache, eager, self.trace, dev, model), Plan(be, self.cache, eager, self.trace, dev, model)
        self.other, self.embedding = None, False

    def call(self, st, traced):
        del self.trace[:]
        self.dev.begin_call()
        return getattr(self, st.call)(**st.args), list(self.trace)

    def close(self):
        pass

    def Eval(self, tokens, past):
        self.ml.eval(tokens, past)
        return {"logits": logits(self.ml.scratch.r(len(tokens) - 1))}

    def EmbeddingEval(self, tokens, past):
        self.embedding = True
        res = self.Eval(tokens, past)
        res["embedding"] = _u64([mix(int(res["logits"][0]), 7)])
        return res

    def Decode(self, first, past, n):
        p = self.res
        p.ensure_out(n)
        p.resident(first, past, n, False, 0)
        return {"ids": _u32([p.out.r(i) for i in range(n)]), "logits": logits(p.scratch.r(0))}

    def DecodeSplit(self, first, past, counts, keep):
        from session_ref import swap_positions
        ids, res = [], None
        for n in counts:
            res = self.Decode(first, past, n)
            ids += [int(t) for t in res["ids"]]
            past, first = swap_positions(past, n, self.ctx, keep), ids[-1]
        return {"ids": _u32(ids), "logits": res["logits"]}

    def SampleDecode(self, prompt, n, topK, seed):
        p = self.res
        p.ensure_out(n)
        p.arm_sampler(prompt, self.ctx, topK, seed)
        p.eval(prompt, 0)
        p.sp.update(token=0, past=len(prompt) - 1, step=0)
        tok = sample(p.scratch.r(len(prompt) - 1), p.ss, p.ring, 0, p.variant())
        p.out.w(0, tok)
        if n > 1:
            p.resident(tok, len(prompt), n - 1, True, 1)
        return {"ids": _u32([p.out.r(i) for i in range(n)])}

    def Score(self, tokens, past):
        p = self.res
        p.score_cap = max(p.score_cap, len(tokens))
        if self.be.mutant == "detour_leaves_row" and past > 0:
            self.cache.rows[past - 1] = mix(13, past)
        p.eval(tokens, past) if len(tokens) > 1 else p.k_rows(p.scratch, tokens, past)
        return {"rows": _u64([[p.scratch.r(i), greedy(p.scratch.r(i))] for i in range(len(tokens))])}

    def Verify(self, tokens, past):
        p, n = self.res, len(tokens)
        p.ensure_rows(n)
        p.ensure_out(n)
        self.trace.append(f"k_attention/rows/hd64/n{n}")
        p.k_rows(p.scratch, tokens, past)
        ids = [greedy(p.scratch.r(i)) for i in range(n)]
        a = 0
        while a + 1 < n and tokens[a + 1] == ids[a]:
            a += 1
        return {"ids": _u32(ids[:a + 1]), "accepted": _u32([a]), "logits": logits(p.scratch.r(a))}

    def DecodeLookup(self, first, past, n, draft_max, ngram_max=3, ngram_min=1, corpus=None):
        ids, st, passes = self.res.lookup(first, past, n, draft_max, ngram_max, ngram_min, corpus, False, 0)
        return {"ids": _u32(ids), "logits": logits(self.cache.chain(past + n - 1)), "stats": _u32([st]), "passes": _u32(passes).reshape(-1, 2)}

    def SampleDecodeLookup(self, prompt, n, draft_max, ring, topK, seed, ngram_max=3, ngram_min=1):
        p = self.res
        p.ensure_out(n)
        p.arm_sampler(prompt, ring, topK, seed)
        p.eval(prompt, 0)
        tok = sample(p.scratch.r(len(prompt) - 1), p.ss, p.ring, 0, p.variant())
        p.out.w(0, tok)
        ids, st, passes = p.lookup(tok, len(prompt), n - 1, draft_max, ngram_max, ngram_min, None, True, 1)
        return {"ids": _u32([tok] + ids), "stats": _u32([st]), "passes": _u32(passes).reshape(-1, 2)}

    def SetKeepCount(self, keep):
        self.ml.keep = self.res.keep = keep
        return {}

    def CacheImage(self, pos):
        return {"k": _u64(self.cache.rows[:pos]), "v": _u64([r ^ 1 for r in self.cache.rows[:pos]])}

    def OpenOther(self, ctx, tokens, past):
        self.other = ToySolo(self.be, ctx, self.eager, Dev(self.be, None, False))
        return self.other.Eval(tokens, past)

    def CloseOther(self):
        self.other = None
        return {}


class ToyBatch:
    """`pods` caches with a plan each; the ticks run on pod 0's plan.  batch_tick_unchecked's warm flag, graph and staleness key; the feed schedule's
    passes; the sharing groups of lh_batch_fork; the pods x R lookup passes."""

    def __init__(self, be, ctx, pods, eager, dev):
        self.be, self.ctx, self.B, self.dev, self.trace = be, ctx, pods, dev, []
        self.use_graph = not eager
        self.caches = [Cache(ctx) for _ in range(pods)]
        self.plans = [Plan(be, c, eager, self.trace, dev) for c in self.caches]
        self.plans[0].ensure_rows(pods)
        self.pos, self.tok = [0] * pods, [0] * pods
        self.sampling, self.ss, self.ring, self.ring_cap, self.ring_size, self.smp_topk = False, [None] * pods, None, 0, 0, 0
        self.warm, self.graph_, self.seen = False, None, 0
        self.feed_cap = 0
        self.gid, self.glen, self.next_gid, self.sent = [None] * pods, [0] * pods, 0, None
        self.spec_warm, self.spec_graph, self.spec_seen = set(), None, 0

    def call(self, st, traced):
        del self.trace[:]
        self.dev.begin_call()
        return getattr(self, st.call)(**st.args), list(self.trace)

    def close(self):
        pass

    def scratch_gen(self):
        return sum(p.scratch_gen for p in self.plans)

    def ensure_splitk(self, n):
        self.dev.ensure_splitk(n)

    # ---- sharing groups ----
    def leave(self, pod):
        g = self.gid[pod]
        if g is None:
            return
        self.gid[pod], self.glen[pod] = None, 0
        rest = [i for i in range(self.B) if self.gid[i] == g]
        if len(rest) == 1:
            self.gid[rest[0]], self.glen[rest[0]] = None, 0

    def written(self, pod, pos):
        if self.gid[pod] is not None and pos < self.glen[pod]:
            self.leave(pod)

    def share_info(self):
        group = [min([j for j in range(self.B) if self.gid[j] == self.gid[i]]) if self.gid[i] is not None else i for i in range(self.B)]
        return {"group": _u32(group), "length": _u32(self.glen)}

    def Fork(self, src, dst, n_pos):
        for d in dst:
            self.caches[d].rows[:n_pos], self.caches[d].hist[:n_pos] = self.caches[src].rows[:n_pos], self.caches[src].hist[:n_pos]
        if self.gid[src] is None or self.glen[src] != n_pos:
            self.leave(src)
            self.gid[src], self.glen[src], self.next_gid = self.next_gid, n_pos, self.next_gid + 1
        for d in dst:
            self.leave(d)
            self.gid[d], self.glen[d] = self.gid[src], n_pos
        return self.share_info()

    # ---- ticks ----
    def k_tick(self, scratch, ring, variant, sampling, broken=0):
        for i in range(self.B):
            self.caches[i].write(self.pos[i], self.tok[i])
            scratch.w(i, self.caches[i].chain(self.pos[i]) ^ broken)
            c = scratch.r(i)
            self.tok[i] = sample(c, self.ss[i], ring, i * self.ring_cap, variant) if sampling else greedy(c)

    def Tick(self, n=1):
        out = []
        for _ in range(n):
            for i in range(self.B):
                self.written(i, self.pos[i])
            env = self.be.env
            row_attn = env.get("LLAMAHIP_SHARE_ROW_ATTN") == "1"
            table = None if row_attn or self.ctx <= 256 else tuple((g, ln) for g, ln in zip(self.gid, self.glen))
            if table != self.sent and self.ctx > 256:
                self.trace.append("share_table/b1")
                self.sent = table
            shared = bool(table) and any(g is not None for g in self.gid)
            now = self.dev.stream_key()
            key = (self.dev.splitk_gen, self.scratch_gen(), self.sampling, env.get("LLAMAHIP_SAMPLE_PER_POD") == "1", shared,
                   int(env.get("LLAMAHIP_SHARE_QB", 4)) if shared else 0, now)
            if self.seen != now:   # f16_stream_sync
                self.seen = now
                if self.be.mutant != "warm_not_cleared":
                    self.warm = False
            bufs = (self.plans[0].scratch, self.ring, "small" if self.smp_topk <= 64 else "large", self.sampling, 0)
            if not self.use_graph or not self.warm:
                self.warm = True
                self.dev.lds.add(self.dev.variant())   # an eager launch sets the kernel's attribute
                self.trace.append(f"k_attention/rows/hd64/n{self.B}")
            else:
                if self.graph_ and self.graph_[0] != key:
                    self.graph_ = None
                if not self.graph_:
                    self.trace.append(f"k_attention/rows/hd64/n{self.B}")
                    # a kernel whose first launch stands inside a capture runs without its attribute: the graph computes garbage
                    self.graph_ = (key, bufs[:4] + (0 if self.dev.variant() in self.dev.lds else POISON,))
                bufs = self.graph_[1]
            self.k_tick(*bufs)
            self.pos = [p + 1 for p in self.pos]
            out.append(list(self.tok))
        res = {"ids": _u32(out[-1])}
        if self.sampling:
            res.update(self.SamplerState())
        return res

    def Prompt(self, prompts):
        self.sampling = False
        for i, p in enumerate(prompts):
            self.written(i, 0)
            self.plans[i].eval(p, 0) if len(p) > 1 else self.plans[i].k_rows(self.plans[i].scratch, p, 0)
            self.tok[i], self.pos[i] = greedy(self.plans[i].scratch.r(len(p) - 1)), len(p)
        return {"ids": _u32(self.tok)}

    def Set(self, tokens, past):
        self.tok, self.pos = list(tokens), list(past)
        for i in range(self.B):
            self.written(i, past[i])
        return {}

    def Feed(self, tokens, past):
        """feed_schedule: pods of FEED_SOLO_MIN rows and more evaluate on their own plan, the others' rows are packed into passes of FEED_PASS_ROWS on pod 0's."""
        rows = [(i, j) for i, t in enumerate(tokens) if 0 < len(t) < FEED_SOLO_MIN for j in range(len(t))]
        if rows:
            self.plans[0].ensure_rows(FEED_PASS_ROWS)
            self.feed_cap = max(self.feed_cap, len(rows))
        last = np.zeros((self.B, 8), dtype=np.uint64)
        ids, wimg = [0xFFFFFFFF] * self.B, 0
        for i, t in enumerate(tokens):
            if len(t) >= FEED_SOLO_MIN:
                self.trace.append(f"feed_pass/solo/n{len(t)}")
                self.written(i, past[i])
                self.plans[i].eval(t, past[i])
                self.ensure_splitk(len(t))
        for k in range(0, len(rows), FEED_PASS_ROWS):
            chunk = rows[k:k + FEED_PASS_ROWS]
            self.trace.append(f"feed_pass/batched/n{len(chunk)}")
            self.trace.append(f"k_attention_seg/hd64/qb4/n{len(chunk)}")
            wimg = self.dev.weights("rows", "M")   # (a feed pass reads the image, or the halves under the switch)
            if len(chunk) > 16:
                self.ensure_splitk(len(chunk))
            for i, j in chunk:
                self.written(i, past[i] + j)
                self.caches[i].write(past[i] + j, tokens[i][j])
        for i, t in enumerate(tokens):
            if t:
                c = self.caches[i].chain(past[i] + len(t) - 1) ^ (wimg if len(t) < FEED_SOLO_MIN else 0)
                self.tok[i], self.pos[i], ids[i], last[i] = greedy(c), past[i] + len(t), greedy(c), logits(c)
        return {"ids": _u32(ids), "last": last}

    # ---- sampler ----
    def SetSampler(self, topK, seed, ring):
        if ring > self.ring_cap:
            if self.ring:
                self.ring.free()
            self.ring, self.ring_cap, self.graph_ = Buf(self.B * ring), ring, None
            fresh_ring = True
        else:
            fresh_ring = False
        if (topK <= 64) != (self.smp_topk <= 64):
            self.graph_ = None
        self.smp_topk, self.ring_size = topK, ring
        if not (self.be.mutant == "ring_not_reinit" and ring < self.ring_cap and not fresh_ring):
            for i in range(self.B * self.ring_cap):
                self.ring.w(i, 0)
        self.ss = [{"topK": topK, "seed": seed, "draw": 0, "ring_size": ring, "ring_pos": 0} for _ in range(self.B)]
        self.sampling = True
        return self.SamplerState()

    def ClearSampler(self):
        self.sampling = False
        return {}

    def SamplerState(self):
        rings = [[self.ring.r(i * self.ring_cap + j) for j in range(self.ring_size)] for i in range(self.B)]
        return {"rings": _u32(rings), "ring_pos": _u32([s["ring_pos"] for s in self.ss]), "draws": _u64([s["draw"] for s in self.ss])}

    # ---- lookup passes of pods x R rows ----
    def _lookup(self, first, past, n, draft_max, ngram_max, ngram_min, smp):
        R, p0 = draft_max + 1, self.plans[0]
        p0.ensure_rows(self.B * R)
        self.tok, self.pos = list(first), list(past)
        for i in range(self.B):
            self.written(i, past[i])
        ids, passes = [[] for _ in range(self.B)], [[] for _ in range(self.B)]
        while any(len(x) < n for x in ids):
            now = self.dev.stream_key()
            key = (R, (draft_max, ngram_max, ngram_min), self.dev.splitk_gen, self.scratch_gen(), smp,
                   (self.smp_topk <= 64, id(self.ring), self.ring_cap) if smp else (), now)
            if self.spec_seen != now:   # f16_stream_sync
                self.spec_warm.clear()
                self.spec_seen = now
            wimg = self.dev.weights("rows", "M")   # (a pass of pods x R rows reads the image or the halves; a replayed graph holds its own fills)
            bufs = (p0.scratch, self.ring, "small" if self.smp_topk <= 64 else "large")
            if not self.use_graph or self.B * R not in self.spec_warm:
                self.spec_warm.add(self.B * R)
                self.trace.append(f"k_attention/rows/hd64/n{self.B * R}")
            else:
                if self.spec_graph and self.spec_graph[0] != key:
                    self.spec_graph = None
                if not self.spec_graph:
                    self.trace.append(f"k_attention/rows/hd64/n{self.B * R}")
                    self.spec_graph = (key, bufs)
                bufs = self.spec_graph[1]
            scratch, ring, variant = bufs
            for i in range(self.B):
                left = n - len(ids[i])
                if not left:
                    continue
                m = min(1 + mix(self.caches[i].chain(max(self.pos[i] - 1, 0)), R) % R, left)
                for r in range(m):
                    self.caches[i].write(self.pos[i], self.tok[i])
                    scratch.w(i * R + r, self.caches[i].chain(self.pos[i]) ^ wimg)
                    c = scratch.r(i * R + r)
                    self.tok[i] = sample(c, self.ss[i], ring, i * self.ring_cap, variant) if smp else greedy(c)
                    ids[i].append(self.tok[i])
                    self.pos[i] += 1
                passes[i].append((R - 1, m - 1))
        width = max(len(p) for p in passes)
        pp = np.full((self.B, width, 2), 0xFFFFFFFF, dtype=np.uint32)
        for i, p in enumerate(passes):
            pp[i, :len(p)] = _u32(p)
        stats = [[len(p), R, sum(x[0] for x in p), sum(x[1] for x in p), 0] for p in passes]
        lg = np.stack([logits(self.caches[i].chain(self.pos[i] - 1)) for i in range(self.B)])
        return {"ids": _u32(ids), "logits": lg, "stats": _u32(stats), "passes": pp}

    def DecodeLookup(self, first, past, n, draft_max, ngram_max=3, ngram_min=1):
        return self._lookup(first, past, n, draft_max, ngram_max, ngram_min, False)

    def DecodeSampleLookup(self, first, past, n, draft_max, ngram_max=3, ngram_min=1):
        res = self._lookup(first, past, n, draft_max, ngram_max, ngram_min, True)
        res.update(self.SamplerState())
        return res

    def CacheImage(self, pos):
        rows = [r for i in range(self.B) for r in self.caches[i].rows[:pos[i]]]
        return {"k": _u64(rows), "v": _u64([r ^ 1 for r in rows])}

    def OtherBatch(self, pods, prompts, ticks):
        o = ToyBatch(self.be, self.ctx, pods, not self.use_graph, Dev(self.be, None, False))
        ids = [list(o.Prompt(prompts)["ids"])] + [list(o.Tick()["ids"]) for _ in range(ticks)]
        return {"ids": _u32(ids)}


class ToyPair:
    """A draft pair: two contexts (a cache and two plans each) on ONE device - its switch, its split-K buffer, its image, whose slots both models' matrices pass through -
    and the draft runs, which work on the TARGET's speculative state and run the draft's steps eagerly (spec_decode_draft)."""

    def __init__(self, be, ctx, eager, dev):
        self.be, self.ctx, self.eager, self.dev, self.trace = be, ctx, eager, dev, []
        self.target = ToySolo(be, ctx, eager, dev, "T", self.trace)
        self.draft = ToySolo(be, ctx, eager, dev, "D", self.trace)
        self.replaced = 0

    def call(self, st, traced):
        del self.trace[:]
        self.dev.begin_call()
        side, _, name = st.call.rpartition(".")
        return getattr(getattr(self, side) if side else self, name)(**st.args), list(self.trace)

    def close(self):
        pass

    def DecodeDraft(self, first, past, n, draft_len):
        p, d, R = self.target.res, self.draft.res, draft_len + 1
        p.ensure_rows(R)
        p.ensure_out(n)
        d.ensure_out(8)
        if self.be.mutant != "draft_leaves_smp":
            p.spec_smp = False
        p.sp.update(token=first, past=past, step=0)
        passes = []
        while p.sp["step"] < n:   # (no captured pass: the draft's steps stand between the target's passes, all of it eager)
            self.trace.append(f"k_attention/rows/hd64/n{R}")
            m = p.k_spec(p.scratch, p.out, p.ring, p.variant(), R, p.spec_smp, 0, n - p.sp["step"], self.draft.cache)
            passes.append((R - 1, m - 1))
        ids = [p.out.r(i) for i in range(n)]
        st = [len(passes), R, sum(x[0] for x in passes), sum(x[1] for x in passes), 0]
        return {"ids": _u32(ids), "logits": logits(self.target.cache.chain(past + n - 1)), "stats": _u32([st]), "passes": _u32(passes).reshape(-1, 2)}

    def ReplaceDraft(self):
        for pl in (self.draft.ml, self.draft.res):
            for b in (pl.scratch, pl.out, pl.ring):
                if b:
                    b.free()
        if self.be.mutant == "replace_frees_out" and self.target.res.out:
            self.target.res.out.free()
            self.target.res.out = Buf(self.target.res.out_cap)
        self.replaced += 1
        self.draft = ToySolo(self.be, self.ctx, self.eager, self.dev, f"D{self.replaced}", self.trace)
        return {}

    def CacheImage(self, pos, draft_pos):
        t, d = self.target.CacheImage(pos), self.draft.CacheImage(draft_pos)
        return {"k": t["k"], "v": t["v"], "draft_k": d["k"], "draft_v": d["v"]}


class ToyBackend:
    def __init__(self, mutant=None, poison=True):
        self.mutant, self.env, self.poison = mutant, {}, poison

    def setenv(self, name, value):
        if value is None:
            self.env.pop(name, None)
        else:
            self.env[name] = value

    def restore_env(self):
        self.env.clear()

    def open(self, script, weights, eager, role="long"):
        eager = eager and self.mutant != "twin_not_eager"
        dev = Dev(self, weights, self.poison and role == "long")   # (the image is poisoned in front of the long-lived object's steps only)
        if script.kind == "pair":
            return ToyPair(self, script.ctx, eager, dev)
        return ToySolo(self, script.ctx, eager, dev) if script.kind == "solo" else ToyBatch(self, script.ctx, script.pods, eager, dev)
