"""Scenarios at the ends of the int32 token range, and what the oracle must show for each.

A node word of a snapshot record is a full signed 32-bit value: cl_add_node takes any int32, a
negative one included, as long as the positive initial tokens sum to at most INT32_MAX.  Device code
that reads such a word is correct only if it sign-extends it and accumulates at 64 bits
(Stat4::add_i32, quantity_value(SEL_NODE), snapshot_key, the crosstab's sum of products, order_key's
sign flip, the signed balance check of send_one, the trace's token column).  The scenarios here
reach those values; all use the complete digraph on N1..N3.

SIGNED: N1 2147400000, N2 -2147483648, N3 83647 -- the positive sum is exactly INT32_MAX, the total
is -1; payloads up to 65,535.  `send N3 N1 18300` succeeds only where N1's 257 has already arrived
at N3, so about half the instances end with FATAL_INSUFFICIENT_TOKENS.  N2 stays at INT32_MIN in
some instances of snapshot 2; the true sum of N2 squared and of N1 * N2 over a batch need more than
64 bits, so the wrapped words of the statistics and of the crosstab are exercised.

MAXED: N1 2147418112, N2 65535, N3 -7.  N2 sends all it has to N1, which reaches INT32_MAX in the
instances where the packet has arrived before the snapshot records N1.

The instance-per-lane kernel admits payloads below 128 only (cl_jit.cpp lanes_fit), so a forced
ENGINE_LANES refuses both programs with E_LIMIT.  SIGNED_LANES and MAXED_LANES are the same programs
event for event with every payload scaled below 128 and the initial tokens moved so that the same
ends are reached (positive sum INT32_MAX, N2 at INT32_MIN, N1 at INT32_MAX, the same send that
depends on an arrival); they are what runs where ENGINE_LANES is forced.

DEBT: N1 100, N2 -3, N3 2147483547.  Neither program above sends from a node whose balance is
negative, so the sign of the balance check itself (node.go:113, `tokens < n`) would not show in
them.  Here N2 sends 0 tokens after one tick: the send is fatal where N1's 5 tokens have not yet
arrived (-3 < 0) and succeeds where they have, on either exec kernel (payloads below 128).

signed(), maxed() and debt() assert the regime on the oracle rows alone, for the variant asked
for; a test that runs a scenario gets its rows from them, so that it cannot pass without having
reached the values it is about.

Not covered: a channel's token sum above 2^31.  It needs more than 32,768 recorded messages on one
channel (payloads are at most 65,535), which no batch of test size reaches.
"""
import numpy as np

import oracle as O
from selectcheck import scenario

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
I64_MIN = -2**63

LINKS = "N1 N2\nN2 N1\nN1 N3\nN3 N1\nN2 N3\nN3 N2\n"      # test_order_gpu.WIDE_TOP's link lines

SIGNED_TOP = "3\nN1 2147400000\nN2 -2147483648\nN3 83647\n" + LINKS
SIGNED_EVENTS = ("send N1 N2 65535\nsend N1 N3 257\nsend N3 N2 1\ntick 1\nsend N1 N2 3000\nsend N3 N1 65535\nsnapshot N3\n"
                 "send N3 N1 5\nsend N1 N2 1\ntick 2\nsnapshot N1\nsend N3 N1 18300\nsend N1 N3 40000\ntick 1\n"
                 "snapshot N2\n")
MAXED_TOP = "3\nN1 2147418112\nN2 65535\nN3 -7\n" + LINKS
MAXED_EVENTS = "send N2 N1 65535\ntick 3\nsnapshot N3\ntick 1\nsnapshot N1\n"

# payloads below 128: N3 holds 163 - 1 - 127 - 5 = 30 before `send N3 N1 80`, 87 where N1's 57 has arrived
SIGNED_LANES_TOP = "3\nN1 2147483484\nN2 -2147483648\nN3 163\n" + LINKS
SIGNED_LANES_EVENTS = ("send N1 N2 127\nsend N1 N3 57\nsend N3 N2 1\ntick 1\nsend N1 N2 30\nsend N3 N1 127\nsnapshot N3\n"
                       "send N3 N1 5\nsend N1 N2 1\ntick 2\nsnapshot N1\nsend N3 N1 80\nsend N1 N3 100\ntick 1\n"
                       "snapshot N2\n")
MAXED_LANES_TOP = "3\nN1 2147483520\nN2 127\nN3 -7\n" + LINKS
MAXED_LANES_EVENTS = "send N2 N1 127\ntick 3\nsnapshot N3\ntick 1\nsnapshot N1\n"

DEBT_TOP = "3\nN1 100\nN2 -3\nN3 2147483547\n" + LINKS
DEBT_EVENTS = ("send N1 N2 5\ntick 1\nsnapshot N3\nsend N2 N3 0\ntick 1\nsend N2 N3 2\nsend N2 N1 0\ntick 1\n"
               "snapshot N2\n")

N1, N2, N3 = 0, 1, 2        # node ranks


def signed_texts(lanes=False):
    return (SIGNED_LANES_TOP, SIGNED_LANES_EVENTS) if lanes else (SIGNED_TOP, SIGNED_EVENTS)


def maxed_texts(lanes=False):
    return (MAXED_LANES_TOP, MAXED_LANES_EVENTS) if lanes else (MAXED_TOP, MAXED_EVENTS)


def initial_tokens(top):
    return [int(line.split()[1]) for line in top.split("\n")[1:4]]


def true_sum(x, y=None):
    """The sum of x * y (x * x by default) in Python integers: no wrap."""
    y = x if y is None else y
    return sum(int(a) * int(b) for a, b in zip(x, y))


def signed(n, lanes=False):
    """(rows, keys) of SIGNED (SIGNED_LANES) at n instances, its regime asserted on the oracle."""
    top, events = signed_texts(lanes)
    init = initial_tokens(top)
    assert sum(t for t in init if t > 0) == INT32_MAX and sum(init) == -1 and init[N2] == INT32_MIN
    rows, keys = scenario(top, events, n)
    ok = rows.status == O.OK
    assert rows.n_sids == 3 and set(np.unique(rows.status).tolist()) == {O.OK, O.FATAL_INSUFFICIENT_TOKENS}
    assert 0 < int(ok.sum()) < n                                            # mixed statuses
    assert all(np.array_equal(d, ok) for d in rows.done)                    # every snapshot completes where OK
    n1 = np.concatenate([rows.node[sid][ok, N1] for sid in range(3)])
    n2 = np.concatenate([rows.node[sid][ok, N2] for sid in range(3)])
    assert int(n2.min()) == INT32_MIN and int(n2.max()) < -2**31 + 2**17    # INT32_MIN occurs as a node value
    assert 2**31 - 2**18 < int(n1.min()) < int(n1.max()) <= INT32_MAX       # N1 within 2^18 of the top
    last = rows.node[2][ok, N2]
    assert (last == INT32_MIN).any() and (last != INT32_MIN).any()
    assert max(int(rows.ch_msgs[sid].max()) for sid in range(3)) >= 2
    if not lanes:
        assert max(int(rows.ch_tok[sid].sum(axis=1).max()) for sid in range(3)) > 65535   # in flight: past 16 bits
    # the words that wrap: a sum of squares past 2^64, a sum of products past 2^63; a plain sum past 2^32
    a, b = rows.node[0][ok, N1], rows.node[2][ok, N2]
    assert true_sum(b) >= 2**64 and abs(true_sum(a, b)) >= 2**63 and abs(int(b.sum())) >= 2**32
    return rows, keys


def maxed(n, lanes=False):
    """(rows, keys) of MAXED (MAXED_LANES) at n instances, its regime asserted on the oracle."""
    top, events = maxed_texts(lanes)
    start, sent, _ = initial_tokens(top)
    assert start + sent == INT32_MAX
    rows, keys = scenario(top, events, n)
    assert (rows.status == O.OK).all() and rows.n_sids == 2 and rows.done[0].all() and rows.done[1].all()
    for sid in range(2):
        v = rows.node[sid][:, N1]
        assert set(np.unique(v).tolist()) == {start, INT32_MAX}             # INT32_MAX occurs as a node value
        arrived = v == INT32_MAX
        assert 0 < int(arrived.sum()) < n
        assert (rows.ch_tok[sid].sum(axis=1) == np.where(arrived, 0, sent)).all()      # ... or the payload in flight
        assert (rows.node[sid][:, N3] == -7).all() and (rows.node[sid][:, N2] == 0).all()
    return rows, keys


def debt(n):
    """(rows, keys) of DEBT at n instances, its regime asserted on the oracle."""
    init = initial_tokens(DEBT_TOP)
    assert sum(t for t in init if t > 0) == INT32_MAX and init[N2] < 0
    rows, keys = scenario(DEBT_TOP, DEBT_EVENTS, n)
    ok = rows.status == O.OK
    assert set(np.unique(rows.status).tolist()) == {O.OK, O.FATAL_INSUFFICIENT_TOKENS} and rows.n_sids == 2
    # the first send from N2 decides: its balance is -3 or 2, the payload 0
    arrived = np.array([r.node_tokens()["N2"] != -3 for r in keys.refs])
    assert np.array_equal(arrived, ok) and 0 < int(ok.sum()) < n
    assert all(np.array_equal(d, ok) for d in rows.done)
    assert (rows.node[1][ok, N2] == 0).all() and set(np.unique(rows.node[0][ok, N2]).tolist()) <= {0, 2}
    return rows, keys
