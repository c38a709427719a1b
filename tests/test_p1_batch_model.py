"""The batched loop of S's pre-aggregating code pass (k_chunk_codes_pipe BATCH,
csrc/phj_partition.h), restated in Python and run under random interleavings
of many workgroups (CPU; the kernel's GPU tests are tests/test_gpu_p1_batch.py).

A loop iteration is one input tile: its k kept codes (0 <= k <= T) get the
next indices g among the workgroup's kept codes and go to ring slot g mod 2T;
batch b = indices [bT, (b + 1)T) lies in half b & 1. A code past the batch
being filled is held back until the pending batch is written out of that
half. Once the ring holds T unsorted codes the batch closes: one claim per
digit on the shard's chain cursors (with the hint), the reserved chunk of the
workgroup's b-th tile. The claims are resolved in the very next iteration
(publishes, then waits, then the write-out), batch or none; after the last
tile the leftover closes as a partial batch and is resolved one iteration on.
The chunk protocol itself is tests/test_chunk_protocol.py's with kPipeRes = 1.

Checked for every interleaving: the ring never holds more than 2T codes and no
live slot is overwritten; at most one batch is claimed per iteration; every
batch is resolved in the next iteration; no workgroup blocks forever; every
chunk of a chain has one id that all runs agree on; ids stay within the pool
and no id is shared; every claimed slot is written exactly once; the kept
codes come out as the same multiset per digit.
"""
import random
from collections import Counter

import pytest

RES = 1   # kPipeRes


class Shard:
    def __init__(self, nb, T, per):
        self.nb, self.T, self.per = nb, T, per
        self.cursor = [0] * nb
        self.hint = [None] * nb          # (j, id_j, id_j1) or None (= (0, static0, static1))
        self.tab = [dict() for _ in range(nb)]
        self.pool = 0
        self.dyn_base = 2 * nb + RES * per
        self.stride = 2 * nb + RES * per + per + nb + 1
        self.writes = [dict() for _ in range(nb)]     # chain position -> (chunk id, offset, code)
        self.chunk_ids = [dict() for _ in range(nb)]  # chunk index -> id (every run's view must agree)
        self.kept = [Counter() for _ in range(nb)]    # what the fronts kept, per digit


class WG:
    """One workgroup: tiles = [(tile index, [kept codes as (digit, tag)])]."""

    def __init__(self, shard, tiles, late_hints=False):
        self.s, self.tiles, self.late = shard, tiles, late_hints
        T = shard.T
        self.ring = [None] * (2 * T)
        self.it = 0            # iteration
        self.gtot = 0          # kept codes appended
        self.uns = 0           # ... not yet in a closed batch
        self.nbat = 0
        self.pend = None       # (iteration it closed in, half, count, claims[d] = [v0, c, hint, start])
        self.phase = 0
        self.max_occ = 0
        self.batches_at = []   # iteration of every close

    def done(self):
        return self.phase == 3

    def step(self):
        """One action; False when blocked (a wait in the protocol)."""
        S, T = self.s, self.s.T
        if self.phase == 0:     # front: part 1 of the append
            live = self.it < len(self.tiles)
            self.live = live
            self.held = []
            self.k = 0
            if live:
                gsort = self.gtot - self.uns
                for j, code in enumerate(self.tiles[self.it][1]):
                    S.kept[code[0]][code] += 1
                    g = self.gtot + j
                    if g - gsort < T:
                        self.put(g, code)
                    else:
                        self.held.append((g, code))
                self.k = len(self.tiles[self.it][1])
            self.phase = 1
            return True
        if self.phase == 1:     # the pending batch: protocol (may wait), then its write-out
            if self.pend is not None:
                closed_in, half, count, claims = self.pend
                assert closed_in == self.it - 1, "a batch is resolved in the very next iteration"
                if not self.resolve(half, count, claims):
                    return False
                self.pend = None
            self.phase = 2
            return True
        # after barrier A: the count is known; the batch closes or not
        tot = self.uns + self.k
        self.gtot += self.k
        occ = tot + 0   # (the pending batch is written out by now)
        self.max_occ = max(self.max_occ, occ)
        assert occ < 2 * T
        closes = tot >= T if self.live else tot != 0
        bcnt = min(tot, T)
        if closes:
            half = self.nbat & 1
            codes = self.ring[half * T:half * T + bcnt]
            assert all(c is not None for c in codes)
            if tot > T:   # after B1: the held codes go to the other half, written out above
                assert len(self.held) == tot - T
            counts = [0] * S.nb
            for c in codes:
                counts[c[0]] += 1
            by_digit = sorted(codes, key=lambda c: c[0])   # (the LDS scatter: any order inside a digit)
            claims, start = [], 0
            for d in range(S.nb):
                v0 = S.cursor[d]
                S.cursor[d] += counts[d]
                claims.append([v0, counts[d], "late" if self.late else S.hint[d], start])
                start += counts[d]
            self.ring[half * T:half * T + bcnt] = by_digit
            for i in range(bcnt, T):
                self.ring[half * T + i] = None
            res_tile = self.tiles[self.nbat][0]   # the b-th tile's reservation: raises if there are more batches than tiles
            self.pend = (self.it, half, bcnt, claims)
            self.res = [res_tile, 0]
            self.batches_at.append(self.it)
            self.nbat += 1
        for g, code in self.held:
            self.put(g, code)
        self.uns = tot - (bcnt if closes else 0)
        self.it += 1
        if not self.live and self.pend is None:
            assert all(c is None for c in self.ring)
            self.phase = 3
        else:
            self.phase = 0
        return True

    def put(self, g, code):
        slot = g % (2 * self.s.T)
        assert self.ring[slot] is None, "a live ring slot overwritten"
        self.ring[slot] = code

    def resolve(self, half, count, claims):
        S, T = self.s, self.s.T
        if not hasattr(self, "st"):   # publishes, once per batch (no waits)
            self.st = {}
            for d, (v0, c, _h, _s) in enumerate(claims):
                if c == 0:
                    continue
                off, k0, k1 = v0 % T, v0 // T, (v0 + c - 1) // T
                s = k0 if off == 0 else (k1 if k1 != k0 else None)
                if s is None:
                    continue
                if s == 0:
                    S.tab[d][0] = 2 * d
                    S.tab[d][1] = 2 * d + 1
                    self.st[d] = (0, 2 * d + 1)
                else:
                    r = self.res[1]
                    self.res[1] += 1
                    nid = 2 * S.nb + RES * self.res[0] + r if r < RES else S.dyn_base + S.pool
                    if r >= RES:
                        S.pool += 1
                    S.tab[d][s + 1] = nid
                    self.st[d] = (s, nid)
        for d, cl in enumerate(claims):
            if cl[2] == "late":   # the hint load landed at any time up to now
                cl[2] = S.hint[d]
        ids = {}
        for d, (v0, c, h, _s) in enumerate(claims):
            if c == 0:
                continue
            k0, k1 = v0 // T, (v0 + c - 1) // T
            hk, hid, hid1 = h if h is not None else (0, 2 * d, 2 * d + 1)

            def id_of(k):
                if k == 0:
                    return 2 * d
                if k == 1:
                    return 2 * d + 1
                if k == hk:
                    return hid
                if k == hk + 1:
                    return hid1
                return S.tab[d].get(k)
            i0, i1 = id_of(k0), id_of(k1)
            if i0 is None or i1 is None:
                return False   # spin: retried later
            ids[d] = (i0, i1)
        for d, (v0, c, h, start) in enumerate(claims):
            if c == 0:
                continue
            i0, i1 = ids[d]
            k0, k1 = v0 // T, (v0 + c - 1) // T
            if d in self.st and self.st[d][0] != 0:
                s, nid = self.st[d]
                ent = (s, i0 if s == k0 else i1, nid)
                if S.hint[d] is None or ent[0] > S.hint[d][0]:
                    S.hint[d] = ent   # atomicMax on the packed word
            for k, i in ((k0, i0), (k1, i1)):
                assert S.chunk_ids[d].setdefault(k, i) == i, ("two ids for one chunk", d, k)
                assert 0 <= i < S.stride
            for j in range(c):   # the write-out: slot start + j of the sorted batch
                pos = v0 + j
                code = self.ring[half * T + start + j]
                assert code is not None and code[0] == d
                assert pos not in S.writes[d]
                S.writes[d][pos] = (i0 if pos // T == k0 else i1, pos % T, code)
        for i in range(count):
            self.ring[half * T + i] = None
        del self.st
        return True


def kept_counts(rng, T, ntiles, mode):
    """Kept codes per iteration of one workgroup."""
    if mode == "random":
        return [rng.randint(0, T) for _ in range(ntiles)]
    if mode == "zeros":       # runs of iterations that keep nothing
        return [0 if (i // 3) % 2 == 0 else rng.randint(0, T) for i in range(ntiles)]
    if mode == "full":        # a batch closes every iteration
        return [T] * ntiles
    if mode == "exact":       # the ring lands on exactly T, again and again
        return [T // 2] * ntiles
    if mode == "edge":        # unsorted T - 1, then + T: the ring at 2T - 1
        return [T - 1, T, 0, 0, T - 1, T, T, 1, 0][:ntiles] + [rng.randint(0, T) for _ in range(max(0, ntiles - 9))]
    if mode == "sparse":      # fewer than a batch in all: only the drain
        return [rng.randint(0, 1) for _ in range(ntiles)]
    raise ValueError(mode)


def run(seed, nb=6, T=16, W=5, ntiles=60, mode="random", skew=False, late=False):
    rng = random.Random(seed)
    S = Shard(nb, T, ntiles)
    wgs, tag = [], 0
    for w in range(W):
        mine = list(range(w, ntiles, W))
        ks = kept_counts(rng, T, len(mine), mode)
        tiles = []
        for t, k in zip(mine, ks):
            codes = []
            for _ in range(k):
                codes.append((0 if skew else rng.randrange(nb), tag))
                tag += 1
            tiles.append((t, codes))
        wgs.append(WG(S, tiles, late_hints=late and rng.random() < 0.5))
    stuck = 0
    while not all(g.done() for g in wgs):
        g = rng.choice([g for g in wgs if not g.done()])
        if g.step():
            stuck = 0
        else:
            stuck += 1
            assert stuck < 10_000, "deadlock: every live workgroup waits"
    seen = {}
    for d in range(nb):
        assert sorted(S.writes[d]) == list(range(S.cursor[d]))   # every claimed slot written once
        assert Counter(c for _i, _o, c in S.writes[d].values()) == S.kept[d]   # the same multiset per digit
        for k, i in S.chunk_ids[d].items():
            assert seen.setdefault(i, (d, k)) == (d, k), "one id for two chunks"
    for g in wgs:
        assert len(set(g.batches_at)) == len(g.batches_at)        # at most one batch per iteration
        assert g.nbat <= len(g.tiles)
        assert g.it <= len(g.tiles) + 2                           # up to two drain iterations
    return S, wgs


@pytest.mark.parametrize("mode", ["random", "zeros", "full", "exact", "edge", "sparse"])
@pytest.mark.parametrize("seed", range(8))
def test_batched_loop(seed, mode):
    run(seed, mode=mode)


@pytest.mark.parametrize("seed", range(8))
def test_batched_loop_late_hints_and_skew(seed):
    run(seed, late=True)
    run(seed, skew=True, late=True, W=7, ntiles=84, mode="full")
    run(seed, skew=True, W=7, ntiles=84)


@pytest.mark.parametrize("seed", range(6))
def test_batched_loop_many_workgroups(seed):
    run(seed, nb=3, T=8, W=16, ntiles=208)


def test_ring_upper_edge():
    """Unsorted T - 1 plus a tile that keeps T: the ring holds 2T - 1 after the
    pending batch is written out, T - 1 codes wait for its half."""
    _S, wgs = run(0, W=1, ntiles=12, mode="edge")
    assert wgs[0].max_occ == 2 * 16 - 1
