"""What tests/test_gpu_sample_lookup.py (the device) and tests/test_sample_lookup_cpu.py (the checker alone) share: the ring view of a row of a
sampled verify pass in plain Python, written from the text of include/llamahip.h (lh_sample_rows), the logits kinds of the op-level cases, and
the prompts / seeds / corpora of the loop cases - chosen on the CPU so that the checker's own runs contain what the GPU tests assert."""
import numpy as np

HD128 = dict(vocab=512, embd=640, mult=128, heads=5, layers=2)    # tests/test_gpu_speculative.py: both weight types' row kernels are built for it
MODEL_SEED = 4321
SMP = dict(topK=40, topP=0.95, temp=0.8, repeatPenalty=1.1)       # the reference's defaults (main.go:87-90)
N_PREDICT = 48
LOOP_SEEDS = (99, 100)                                            # sampler seeds of the loop cases: the second must give other ids


def kmax(int8):
    return 3 if int8 else 7


def prompt_for(vocab, n, seed=7):
    return [int(t) for t in np.random.default_rng(seed).integers(0, vocab - 1, n)]


def corrupted(corpus, n_prompt, vocab):
    """The replay corpus, wrong at every fifth id behind the prompt: drafts from it are accepted in part."""
    bad = list(corpus)
    for i in range(n_prompt + 5, len(bad), 5):
        bad[i] = (bad[i] + 1) % (vocab - 1)
    return bad


# ---- the lastNTokens ring ---------------------------------------------------------------------------------------------------------------------
def ring_after(appended, ring_size):
    """ring_size zeros (server.go:127-138), then `appended` in order, slot = count % ring_size -> (ring, ring_pos)."""
    ring = [0] * ring_size
    for i, t in enumerate(appended):
        ring[i % ring_size] = int(t)
    return ring, len(appended)


def ring_view(ring, ring_pos, tokens, r):
    """Members of the ring row r of a pass sees (the rule of lh_sample_rows): a slot one of the appends tok[1..r] overwrites is skipped, and every
    append that is the last writer of its slot (append j is, when j + ring_size >= r) adds its id.  The ring is not modified."""
    rs = len(ring)
    base = ring_pos % rs
    members = [int(ring[s]) for s in range(rs) if (s - base) % rs >= r]
    members += [int(tokens[j + 1]) for j in range(r) if j + rs >= r]
    return members


def ring_view_literal(ring, ring_pos, tokens, r):
    """The same by literal sequential appends to a copy."""
    ring = [int(t) for t in ring]
    for j in range(r):
        ring[(ring_pos + j) % len(ring)] = int(tokens[j + 1])
    return ring


# ---- logits of the op-level cases (the kinds of tests/test_gpu_sample.py) ------------------------------------------------------------------------
def logits_of(rng, V, kind):
    x = rng.standard_normal(V).astype(np.float32) * 4
    if kind == "ties":
        x = np.round(x * 2) / 2
    if kind == "neginf":
        x[rng.integers(0, V, V // 3)] = -np.inf
    if kind == "flat":
        x[:] = -0.75
    if kind == "zeros":        # +0 / -0 compare equal in the reference: ids decide
        x[: V // 2] = 0.0
        x[1: V // 2: 2] = -0.0
        x[V // 2:] = -1.0
    return x.astype(np.float32)


def sequential_ids(sample, logits_rows, ring, ring_pos, tokens, draw0):
    """What a multi-row launch must return: one-token sampling calls in order, `sample(logits, ring members, draw) -> id`, row i as call
    draw0 + i over the ring behind tokens[1..i]."""
    return [int(sample(logits_rows[i], ring_view(ring, ring_pos, tokens, i), draw0 + i)) for i in range(len(logits_rows))]
