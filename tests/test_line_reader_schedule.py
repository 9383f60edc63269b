"""The static schedule of the batch transcoder's line reader (LineReader, qoi_decode.hip) never lets a lane run out of bytes.

A turn of the reader's loop is kLinePeriods periods.  Period 0 asks for a whole 128-byte line into the register set if the set is
free; period kLineLand0 + k moves piece k (32 bytes) into the 128-byte ring if the lane holds it and the ring has 32 bytes of room.
A lane consumes at most 10 bytes per period (two five-byte chunks: a QOI_OP_RGBA takes two of a period's four steps; the run-up
takes two steps per period) and may stand still for any number of periods.  init_line leaves 97..128 unread bytes in the ring and
the pieces k0..3 of the next line in the set.  A period's four steps read up to the two dwords behind a cursor that has moved by 10
bytes: 18 unread bytes at the start of every period are enough.  The search below walks every reachable state of that machine with
the constants taken from the source."""
import os
import re
from collections import deque

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qoi_amd", "csrc", "qoi_decode.hip")
MAX_PER_PERIOD, NEEDED = 10, 18


def _constants():
    m = re.search(r"constexpr uint32_t kLinePeriods = (\d+), kLineLand0 = (\d+);", open(SRC).read())
    assert m, "LineReader's schedule constants not found"
    return int(m.group(1)), int(m.group(2))


def _least_unread(periods, land0):
    start = {(0, u, n) for u in range(97, 129) for n in range(0, 4)}
    seen, todo, least = set(start), deque(start), 1 << 30
    while todo:
        t, u, n = todo.popleft()
        if t == 0 and n == 4:
            n = 0                                          # the request; its pieces land from period land0 on
        elif land0 <= t < land0 + 4 and t - land0 == n and u <= 96:
            u, n = u + 32, n + 1
        least = min(least, u)
        for c in range(0, MAX_PER_PERIOD + 1):
            if u - c < -64:
                continue
            s = ((t + 1) % periods, u - c, n)
            if s not in seen:
                seen.add(s); todo.append(s)
    return least


def test_schedule_shape():
    periods, land0 = _constants()
    assert land0 >= 1 and land0 + 3 < periods              # the pieces land behind the request of the same turn, each in a period of its own


def test_no_walk_starves_a_lane():
    periods, land0 = _constants()
    assert _least_unread(periods, land0) >= NEEDED


def test_the_search_finds_a_schedule_that_starves():
    assert _least_unread(8, 4) < NEEDED                    # one period more in flight: a lane at ten bytes per period runs dry
