"""The rule of lh_batch_feed_sample (include/llamahip.h) in plain Python: what a feed does to a pod's sampler state {ring, ring_pos, draw}, and what a
sampled tick does.  tests/test_feed_sample_ref_cpu.py holds it to the checker; tests/test_gpu_feed_sample.py holds the device to it."""
FEED_NEW, FEED_PENDING = 1, 2


class Pod:
    """A pod's sampler state.  ring_pos = ids appended so far (next slot = ring_pos % ring_size); draw = index of the next sampling call."""

    def __init__(self, ring_size, ring=None, ring_pos=0, draw=0):
        self.ring = [0] * ring_size if ring is None else [int(t) for t in ring]
        self.ring_pos, self.draw = int(ring_pos), int(draw)

    def append(self, tok):
        self.ring[self.ring_pos % len(self.ring)] = int(tok)
        self.ring_pos += 1

    def copy(self):
        return Pod(len(self.ring), self.ring, self.ring_pos, self.draw)

    def key(self):
        return (tuple(self.ring), self.ring_pos, self.draw)


def feed_ring(pod, tokens, flags=0):
    """Steps 1 and 2: a NEW pod restarts (ring_size zeros, ring_pos = 0, draw = 0); the fed tokens are appended in order, without the first one
    when it is the pod's PENDING id (its last sampling call appended it)."""
    assert flags in (0, FEED_NEW, FEED_PENDING)
    if flags & FEED_NEW:
        pod.ring, pod.ring_pos, pod.draw = [0] * len(pod.ring), 0, 0
    for t in tokens[1 if flags & FEED_PENDING else 0:]:
        pod.append(t)


def sample_step(pod, sample, logits):
    """Step 3, and a sampled tick: `sample(logits, ring members, draw) -> id` as call `draw` over the ring; the id is appended, ring_pos and draw move on."""
    tok = int(sample(logits, list(pod.ring), pod.draw))
    pod.append(tok)
    pod.draw += 1
    return tok


def feed(pod, tokens, flags, sample, last_row_logits):
    """The whole rule for one fed pod -> the id behind its last fed row (its pending token)."""
    feed_ring(pod, tokens, flags)
    return sample_step(pod, sample, last_row_logits)
