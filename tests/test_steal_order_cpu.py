"""Stealing in the ticketed tile walk of the persistent f16 filter (csrc/mfma_pp.h: steal_victim, steal_item), checked through the
library's host entry point mevi_ip_filter_steal_item -- the same functions the kernel calls.

A workgroup of label g takes its two static items, then draws tickets from its label's counter; when a ticket lies past the
range it moves on to the counters of labels (g + 1) & 7, (g + 2) & 7, ... and leaves after the seventh.  The model below is the
kernel's walk (ip_filter_h16_kernel: next / early / emit, with the ticket of the call after next in flight), one generator per
workgroup that yields at every atomic, run in random interleavings.  Checked: every item of the sweep order is drawn exactly
once, every workgroup terminates after at most seven changes of label, and under `force` no ticketed item is computed by a
workgroup of its own label.
"""
import ctypes
import random

import pytest


@pytest.fixture(scope="module")
def L():
    from mevi_amd import hip
    from mevi_amd.build import build

    build()
    return hip.lib()


def item_of(L, n_items, P, g, hop, ticket):
    """(victim, sweep index or None) of `ticket` drawn by a workgroup of label g that is `hop` labels on."""
    v, s = ctypes.c_int32(-7), ctypes.c_int32(-7)
    r = L.mevi_ip_filter_steal_item(n_items, P, g, hop, ticket, ctypes.byref(v), ctypes.byref(s))
    assert r in (0, 1) and v.value == (g + hop) & 7
    assert (s.value >= 0) == (r == 1)
    return v.value, (s.value if r == 1 else None)


def ranges(n_items):
    q, r = n_items >> 3, n_items & 7
    lens = [q + (g < r) for g in range(8)]
    los = [sum(lens[:g]) for g in range(8)]
    return los, lens


def workgroup(L, n_items, P, g, j0, counters, mode, done, hops):
    """The walk of workgroup j0 of label g; appends (sweep index, victim label or None for a static item) to `done`."""
    los, lens = ranges(n_items)
    thieving = mode != "0" and ((n_items + 7) >> 3) > 2 * P
    state = {"hop": 1 if mode == "force" else 0, "calls": 0, "live": False, "word": 0, "tk": 0}

    def draw():
        v = (g + state["hop"]) & 7
        t = counters[v]
        counters[v] += 1
        return t

    def next_item():
        # returns the item, or None; a generator so that the synchronous draws of a change of label can interleave
        if state["calls"] < 2:
            item = j0 + state["calls"] * P
            state["calls"] += 1
            state["live"] = item < lens[g]
            return (los[g] + item, None) if state["live"] else None
        state["calls"] += 1
        v, s = item_of(L, n_items, P, g, state["hop"], state["word"])
        while s is None and thieving and state["hop"] < 7:
            state["hop"] += 1
            now = draw()
            yield
            v, s = item_of(L, n_items, P, g, state["hop"], now)
            if s is not None:
                state["tk"] = draw()
                yield
        state["live"] = s is not None
        return (s, v) if s is not None else None

    if j0 + P < lens[g]:
        state["tk"] = draw()
        yield
    cur = yield from next_item()
    if cur is not None:
        nxt = yield from next_item()
        while True:
            state["word"] = state["tk"]          # early()
            if state["live"]:                    # emit(): the ticket of the call after next
                state["tk"] = draw()
                yield
            done.append((g, cur))
            if nxt is None:
                break
            cur = nxt
            nxt = yield from next_item()
    hops.append(state["hop"])


SHAPES = [(3, 2), (7, 1), (8, 1), (13, 1), (16, 1), (17, 1), (40, 2), (41, 2), (100, 3), (257, 4), (756, 32), (1001, 5), (3001, 32), (4099, 7)]


@pytest.mark.parametrize("mode", ["0", "1", "force"])
@pytest.mark.parametrize("n_items,P", SHAPES)
def test_every_item_is_drawn_once_in_any_interleaving(L, n_items, P, mode):
    los, lens = ranges(n_items)
    for seed in range(4):
        rng = random.Random(1000 * seed + n_items + P)
        counters, done, hops = [0] * 8, [], []
        live = [workgroup(L, n_items, P, g, j0, counters, mode, done, hops) for g in range(8) for j0 in range(P)]
        if seed == 2:
            rng.shuffle(live)
        steps = 0
        while live:
            # seeds 1, 2: strongly uneven progress -- the first few workgroups of the list get most of the turns (seed 1: label 0's
            # finish before the others have started, and the later labels' in turn; seed 2: in a shuffled order)
            i = min(int(rng.expovariate(0.5)), len(live) - 1) if seed in (1, 2) else rng.randrange(len(live))
            try:
                next(live[i])
            except StopIteration:
                live.pop(i)
            steps += 1
            assert steps < 64 * (n_items + 8 * P) + 10000, "the walk does not terminate"
        assert len(hops) == 8 * P and max(hops) <= 7
        assert sorted(s for _, (s, _) in done) == list(range(n_items))
        stolen = 0
        for g, (s, v) in done:
            if v is None:            # a static item: the workgroup's own range, its first 2 P items
                assert los[g] <= s < los[g] + min(lens[g], 2 * P)
            else:                    # a ticketed item of label v's range
                assert los[v] + 2 * P <= s < los[v] + lens[v]
                stolen += v != g
                if mode == "force":
                    assert v != g
                if mode == "0":
                    assert v == g
        ticketed = sum(max(n - 2 * P, 0) for n in lens)
        if mode == "force":
            assert stolen == ticketed
        if mode == "0" or ticketed == 0:
            assert stolen == 0


def test_ticket_to_item_mapping(L):
    for n_items, P in [(5, 1), (756, 32), (605892, 32)]:
        los, lens = ranges(n_items)
        for g in range(8):
            for hop in range(8):
                v = (g + hop) & 7
                left = max(lens[v] - 2 * P, 0)
                for t in {0, 1, left // 2, max(left - 1, 0)}:
                    want = los[v] + 2 * P + t if t < left else None
                    assert item_of(L, n_items, P, g, hop, t) == (v, want)
                for t in (left, left + 1, 0x7fffffff, 0xffffffff):
                    assert item_of(L, n_items, P, g, hop, t) == (v, None)


def test_bad_arguments_are_refused(L):
    v, s = ctypes.c_int32(0), ctypes.c_int32(0)
    for args in [(0, 32, 0, 0, 0), (1 << 31, 32, 0, 0, 0), (100, 0, 0, 0, 0), (100, 32, 8, 0, 0), (100, 32, -1, 0, 0), (100, 32, 0, 8, 0),
                 (100, 32, 0, -1, 0)]:
        assert L.mevi_ip_filter_steal_item(*args, ctypes.byref(v), ctypes.byref(s)) == -1
    assert L.mevi_ip_filter_steal_item(100, 2, 0, 0, 0, None, None) == 1
