"""The sizes of k_solve_hex's LDS rings (ilqr_amd/csrc/backward_hex.hpp: HexRingSize) compiled for the HOST -- the compile checks the
header's static_asserts for the four rings the library has (double / float, full / compact slots) -- and the protocol they serve, played
through with those sizes:

  * a ring is whole groups of kHexSlotPhases slots and so is a producer round, so a knot's phase is its slot's phase and only a knot of
    phase 0 can be the first one a round has not delivered yet;
  * the compact ring is the most such groups that fit the bytes of 24 full slots (44 of the 45 slots that would), every offset a load
    adds to a lane's address inside a group fits the 16-bit immediate of an LDS instruction;
  * LEAD leaves the producer at least one knot of lead when the index the chain published is STALE = kHexSlotPhases - 1 knots old;
  * chain and producer, interleaved at random, with the chain publishing at phase 0 only and abandoning passes anywhere in the ring:
    the chain always reads the knot it means to read, the producer never writes a slot whose knot the chain has yet to read, and
    neither ever waits for the other for good.

The play is a Python model of the protocol fed the header's constants: it tests the BOUNDS (SLOTS, LEAD, STALE), not HexGate's own code --
next_group's wrap, begin_pass's offset and the addresses that move with them run on the device only and are covered by the bit
comparisons of tests/test_gpu_hex_step_schedule.py."""
import ctypes as C
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "hex_ring_host.hip")
SO = os.path.join(HERE, "native", "libhex_ring_host.so")
HIPCC = "/opt/rocm/bin/hipcc"
RINGS = [(f, c) for f in (0, 1) for c in (0, 1)]
NAMES = ("SLOTS", "LEAD", "STALE", "ELEMS", "real", "TERM", "FIT", "pair_bytes", "Z", "rows")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "ilqr_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO, SRC])
    return C.CDLL(SO)


def sizes(lib, is_float, compact):
    out = (C.c_int * len(NAMES))()
    lib.hex_ring_sizes(is_float, compact, out)
    return dict(zip(NAMES, out))


@pytest.mark.parametrize("is_float,compact", RINGS)
def test_rings_are_whole_groups_that_fit(lib, is_float, compact):
    s, nph, rnd, full = sizes(lib, is_float, compact), lib.hex_slot_phases(), lib.hex_knots_per_round(), lib.hex_full_slots()
    assert nph == 4 and rnd == 16 and full == 24
    assert s["SLOTS"] % nph == 0 and rnd % nph == 0
    assert s["SLOTS"] == (44 if compact else 24) and s["LEAD"] == (27 if compact else 7)
    # the most whole groups that the bytes of 24 full slots hold, the knot-T area beside them
    budget = full * sizes(lib, is_float, 0)["ELEMS"]
    assert s["FIT"] == (budget - s["TERM"]) // s["ELEMS"] and s["SLOTS"] == s["FIT"] // nph * nph
    assert s["SLOTS"] * s["ELEMS"] + s["TERM"] <= budget
    assert 4 * s["pair_bytes"] <= 160 * 1024 - 4096  # four pairs and the kernel's other LDS inside a CU's 160 KB
    # what a load adds to a lane's group address: the slot of the last phase, the furthest element inside it, both elements of a pair
    assert ((nph - 1) * s["ELEMS"] + max(s["Z"], s["rows"]) + 1) * s["real"] < 1 << 16


@pytest.mark.parametrize("is_float,compact", RINGS)
def test_lead_covers_the_stale_index(lib, is_float, compact):
    s, rnd = sizes(lib, is_float, compact), lib.hex_knots_per_round()
    assert s["STALE"] == lib.hex_slot_phases() - 1 == 3
    assert s["LEAD"] == s["SLOTS"] - rnd - 1
    assert s["LEAD"] - s["STALE"] >= 1
    # the last knot of a round that may start, p + LEAD + 15, shares its slot with a knot below the published index p
    assert s["LEAD"] + rnd - 1 - s["SLOTS"] < 0


def play(SLOTS, LEAD, NPH, RND, T, compact, rng, abandon):
    """One chain and its producer (sweep_backward_hex / HexGate), a step of either at a time in random order.  Returns the number of
    rounds the producer was released while the published index was behind the chain."""
    nrounds = (T + 1 + RND - 1) // RND
    N = nrounds * RND
    slot = [None] * SLOTS          # running index of the knot a slot holds
    unread = set()                 # running indices written for the pass the chain is in and not read yet
    pub, rounds_done, started = 0, 0, 0
    c_pass, c_G, have = -1, 0, 0   # chain: pass, next knot, knots delivered
    p_pass, p_round = 0, 0         # producer
    stale_releases = 0
    chain_done = False
    abandon_at = None

    def begin_pass():
        nonlocal c_pass, c_G, have, started, abandon_at
        c_pass += 1
        c_G = have = c_pass * N
        started = c_pass + 1
        unread.clear()
        abandon_at = c_pass * N + rng.randrange(1, T + 1) if (abandon and c_pass < 3) else None

    begin_pass()
    idle = 0
    while not chain_done:
        idle += 1
        assert idle < 10000, "chain and producer wait for each other"
        if rng.random() < 0.5:  # the chain takes knot c_G
            if (c_G - c_pass * N) % NPH == 0:
                pub = c_G
                if c_G >= have:
                    if rounds_done <= c_pass * nrounds + (c_G - c_pass * N) // RND:
                        continue  # blocks (having published the knot it blocks on)
                    have = c_pass * N + ((c_G - c_pass * N) // RND + 1) * RND
            assert c_G < have, "a knot of phase > 0 was the first one missing"
            t = T - (c_G - c_pass * N)
            if not (compact and t == T):
                assert slot[c_G % SLOTS] == c_G, "the chain reads a slot that holds another knot"
            unread.discard(c_G)
            idle = 0
            if c_G == abandon_at:
                begin_pass()
            elif t == 0:
                chain_done = True
            else:
                c_G += 1
        else:  # the producer takes a round
            if p_round == nrounds:  # the pass is swept
                p_pass, p_round = p_pass + 1, 0
            if p_pass > 0 and p_round == 0 and started <= p_pass:
                continue  # a retry pass exists only if the chain starts one
            G0 = p_pass * N + p_round * RND
            if G0 > pub + LEAD:
                continue
            idle = 0
            if started > p_pass + 1:  # the chain has left this pass behind
                p_pass, p_round = p_pass + 1, 0
                continue
            if p_pass == c_pass and pub < c_G:
                stale_releases += 1
            for ks in range(RND):
                t = T - (p_round * RND + ks)
                if t < 0 or (compact and t == T):
                    continue
                g = G0 + ks
                old = slot[g % SLOTS]
                assert old not in unread, "the producer overwrites a knot the chain has yet to read"
                slot[g % SLOTS] = g
                if p_pass == c_pass:
                    unread.add(g)
            rounds_done = p_pass * nrounds + p_round + 1
            p_round += 1
    return stale_releases


@pytest.mark.parametrize("is_float,compact", RINGS[:2])
@pytest.mark.parametrize("abandon", [False, True])
def test_protocol_with_the_index_published_at_phase_0(lib, compact, is_float, abandon):
    s, nph, rnd = sizes(lib, is_float, compact), lib.hex_slot_phases(), lib.hex_knots_per_round()
    rng = random.Random(7 + compact)
    stale = 0
    for T in (1, 3, 15, 16, 17, 46, 93, 130, 499):
        for _ in range(20):
            stale += play(s["SLOTS"], s["LEAD"], nph, rnd, T, bool(compact), rng, abandon)
    assert stale > 0, "no round was released on an index older than the chain's position"
