"""Pairs for the low-memory WFA rung (k_wfa_seg.hip), shared by tests/test_wfa_seg.py (CPU: the premise, on the unmodified reference)
and tests/test_gpu_wfa_seg.py (device parity).  Not a test module."""
import numpy as np

STEPS = [1, 2, 3, 16, 17, 18, 64, 255, 256, 257, 5000]  # around the ring depth (17), around the trim (256), and one that takes no snapshot here


def rand_seq(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes())


def mutate(rng, s, sub, indel):
    """substitutions with probability `sub`, deletions and insertions with `indel` / 2 each"""
    u = rng.random(len(s))
    out = bytearray()
    for c, r in zip(s, u.tolist()):
        if r < sub:
            out.append(int(rng.choice([x for x in b"ACGT" if x != c])))
        elif r < sub + indel / 2:
            continue
        elif r < sub + indel:
            out.append(c)
            out.append(int(rng.choice(list(b"ACGT"))))
        else:
            out.append(c)
    return bytes(out) or b"A"


def mutate_scalar(rng, s, sub, indel):
    """mutate() with one rng draw per base, the draw order of the existing fallback tests (whose cases the route / end-to-end tests regenerate)"""
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < sub:
            out.append(int(rng.choice([x for x in b"ACGT" if x != c])))
        elif r < sub + indel / 2:
            continue
        elif r < sub + indel:
            out.append(c)
            out.append(int(rng.choice(list(b"ACGT"))))
        else:
            out.append(c)
    return bytes(out)


def base_pairs():
    """about 60 (target, query) pairs; deterministic"""
    rng = np.random.default_rng(20251)
    T, Q = [], []

    def add(t, q):
        T.append(t)
        Q.append(q)

    add(b"A", b"A")  # 1 x 1
    add(b"A", b"C")
    s300 = rand_seq(rng, 300)
    add(b"G", s300)  # tl = 1
    add(s300, b"T")  # ql = 1
    s2000 = rand_seq(rng, 2000)
    add(s2000, s2000)  # score 0
    for div in (0.05, 0.1, 0.2, 0.4):  # 5-40 % divergence at 50-3000 bases
        for n in (50, 200, 700, 1500):
            t = rand_seq(rng, n)
            add(t, mutate(rng, t, div * 0.6, div * 0.4))
    for div in (0.05, 0.2):
        t = rand_seq(rng, 3000)
        add(t, mutate(rng, t, div * 0.6, div * 0.4))
    a, x, b = rand_seq(rng, 400), rand_seq(rng, 500), rand_seq(rng, 400)  # one long deletion / insertion: the o2/e2 states run across checkpoints
    add(a + x + b, mutate(rng, a, 0.02, 0.0) + mutate(rng, b, 0.02, 0.0))
    add(mutate(rng, a, 0.02, 0.0) + mutate(rng, b, 0.02, 0.0), a + x + b)
    t = bytearray(rand_seq(rng, 600))  # N against N (raw-byte compare: N matches N)
    for p in (10, 11, 12, 300, 599):
        t[p] = ord("N")
    q = bytearray(mutate(rng, bytes(t), 0.05, 0.02))
    add(bytes(t), bytes(q))
    add(b"N" * 40, b"N" * 37)
    add(rand_seq(rng, 1500), rand_seq(rng, 1500))  # unrelated: the band passes 1024 diagonals, the score 512 (two trims)
    long_ = rand_seq(rng, 1500)
    add(long_[700:800], long_)  # short target in a long query and the reverse: the band grows on one side
    add(long_, long_[200:330])
    add(mutate(rng, long_[100:160], 0.1, 0.1), long_)
    for it in range(24):  # small mixed cases
        n = int(rng.integers(2, 400))
        t = rand_seq(rng, n)
        q = mutate(rng, t, float(rng.choice([0.0, 0.03, 0.1, 0.25])), float(rng.choice([0.0, 0.05, 0.15])))
        if it % 6 == 0:
            q = rand_seq(rng, int(rng.integers(1, 400)))
        if it % 8 == 3:
            t = t[:n // 2] + rand_seq(rng, int(rng.integers(20, 150))) + t[n // 2:]
        add(t, q)
    return T, Q


def checkpoint_pairs(step):
    """two pairs whose scores are meant to be m * step and m * step - 1 (termination at a checkpoint / one score before it): nothing of A^a matches C^b, and for a, b >= 15
    two long gaps (15 + a) + (15 + b) beat every mix with mismatches.  The caller checks the scores with its oracle."""
    m = max(1, -(-60 // step))
    out = []
    for target in (m * step, m * step - 1):
        a = (target - 30) // 2
        out.append((b"A" * a, b"C" * (target - 30 - a), target))
    return out
