"""Topologies and programs for the tests of the lanes kernels' paired senders (cl_lanes.h Pairs:
two senders' out-link head words share the halves of one register).  The kernel sorts the senders
by out-degree (descending, ties by rank) and pairs neighbours; the pairs are noted per topology.
Node ids are in rank order."""

# Five senders, out-degrees 3/2/2/1/1: pairs (A,B), (C,D), (E,-).  E scans beside an inert
# half; both full pairs have unequal degrees.
ODD_TOP = ("5\nA 20\nB 20\nC 20\nD 20\nE 20\n"
           "A B\nA C\nA D\nB A\nB C\nC D\nC E\nD A\nE A\n")
ODD_EVENTS = ("send A B 2\nsend B C 1\nsend C E 3\nsnapshot A\ntick 1\nsend E A 2\nsend D A 1\nsend A D 4\n"
              "snapshot E\ntick 2\nsend C D 1\nsend B A 2\nsend E A 1\nsnapshot C\ntick 1\nsend A C 1\n")

# Five nodes, two of them without out-links, out-degrees 3/2/2/0/0: pairs (A,B), (C,K), (L,-).
# C's partner half never holds a link; the last pair has no link slot at all.
SINKS_TOP = ("5\nA 20\nB 20\nC 20\nK 20\nL 20\n"
             "A B\nA C\nA K\nB A\nB L\nC A\nC K\n")
SINKS_EVENTS = ("send A K 2\nsend B L 1\nsnapshot A\ntick 1\nsend C K 3\nsend C A 1\ntick 2\nsend B A 2\n"
                "snapshot C\ntick 1\nsend A B 1\nsend A K 1\n")

# Out-degrees 3/2/1/1: pairs (I,X), (Y,Z).  Link slot 2 of the first pair is I -> Z alone.
T4_TOP = "4\nI 20\nX 20\nY 20\nZ 20\nI X\nI Y\nI Z\nX Y\nX Z\nY I\nZ I\n"
T4_EVENTS = ("send I Z 3\nsend X Y 2\nsend I X 1\nsend X Z 1\nsnapshot Y\ntick 1\nsend I Z 2\nsend I Y 1\n"
             "send X Y 1\nsnapshot I\ntick 2\nsend Z I 2\nsend I Z 1\nsend X Z 2\nsnapshot X\ntick 1\nsend Y I 1\n")
# the same program cut where packets are in flight on both halves of (I,X) and on I -> Z
T4_PARTS = ("send I Z 3\nsend X Y 2\nsend I X 1\nsend X Z 1\nsnapshot Y\ntick 1\nsend I Z 2\nsend I Y 1\n"
            "send X Y 1\nsnapshot I\n",
            "tick 2\nsend Z I 2\nsend I Z 1\nsend X Z 2\nsnapshot X\ntick 1\nsend Y I 1\n")

# Out-degrees 2/1/1: pairs (P,Q), (R,-).  P -> Q is the low half of the first pair's link slot 0,
# Q -> P its high half.
DEEP_TOP = "3\nP 300\nQ 300\nR 10\nP Q\nP R\nQ P\nR P\n"


def deep_events(deep, other):
    """`other` pushes two packets and pops for two ticks; `deep`'s marker and 126 tokens queue on
    deep -> other: 127 packets, the most a channel may carry; `other` pushes on the partner half
    while that count stands, and 150 ticks pop both.  130 host ops: over the 128 a
    program-specialized kernel takes (each compiles for a minute at that length), so replays run
    the generic kernels."""
    return (f"send {other} {deep} 2\nsend {other} {deep} 3\ntick 2\nsnapshot {deep}\n" + f"send {deep} {other} 1\n" * 126
            + f"send {other} {deep} 5\ntick 150\n")
