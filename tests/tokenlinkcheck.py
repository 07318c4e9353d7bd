"""Topologies and programs for the tests of the lanes kernels' token-carrying in-links (cl_lanes.h
TokIn: a program-specialized kernel has a token path only on the in-links that a send of its
program names) and of the completion check's edge cases.  Node ids are in rank order, so
a node's in-links are numbered by the order of its senders here."""

# I's in-links are Y -> I (0) and Z -> I (1): the two halves of one cursor register.
T4_TOP = "4\nI 20\nX 20\nY 20\nZ 20\nI X\nI Y\nI Z\nX Y\nX Z\nY I\nZ I\n"

# Tokens travel on Z -> I only.  The first is delivered within the six ticks (a delay is at most 4),
# so Z -> I's cursor is 1 when "snapshot I" creates I's record with both in-links recording; two
# more tokens are queued before Z can answer with its marker: I's record has begin cursor 1 and an
# end cursor of at least 3 on Z -> I, and zeros on Y -> I.  "snapshot Y" then has I's record created by the marker
# that arrives on the token-free link itself, with one more token recorded on the other.
SHARED_CURSOR_EVENTS = ("send Z I 1\ntick 6\nsnapshot I\nsend Z I 2\nsend Z I 1\ntick 3\nsnapshot Y\n"
                        "send Z I 3\n")

# R has in-degree and out-degree 4 (records of 8 words, two 16-byte stores).  In-links by sender:
# A (0), B (1), C (2), E (3).  Tokens travel on A -> R and E -> R -- one half of each of R's two
# cursor registers -- and on R -> B.
STAR_TOP = "5\nA 20\nB 20\nC 20\nE 20\nR 20\nA R\nB R\nC R\nE R\nR A\nR B\nR C\nR E\n"
STAR_EVENTS = ("send A R 2\nsend E R 1\ntick 6\nsnapshot B\nsend A R 1\nsend E R 3\nsend R B 2\ntick 2\n"
               "snapshot R\nsend E R 1\nsend A R 4\n")

NO_SEND_EVENTS = "snapshot I\ntick 2\nsnapshot Y\n"
EVERY_CHANNEL_EVENTS = ("send I X 1\nsend I Y 1\nsend I Z 1\nsend X Y 1\nsend X Z 1\nsend Y I 1\nsend Z I 1\n"
                        "snapshot X\ntick 2\nsnapshot Z\n")

# the program's text ends with its drain; ("Y", "I", 3) is then sent as one more event: Y -> I's
# only send stands in the arm of host ops after the last tick op
LAST_ARM_EVENTS = "send I X 2\nsnapshot X\n"
LAST_ARM_SEND = ("Y", "I", 3)

# I holds 20 tokens and sends 25 after two ticks: possible only where Y's 10 arrived by then
INSUFFICIENT_EVENTS = "send Y I 10\nsnapshot X\ntick 2\nsend I X 25\nsnapshot Z\nsend X Z 3\ntick 1\nsend Z I 2\n"
# X has no link to I
UNKNOWN_DEST_EVENTS = "send I X 4\nsnapshot Y\ntick 1\nsend X I 1\nsnapshot I\nsend I Y 2\ntick 2\n"

# four consecutive sends from the four nodes: one OP_SENDS group
GROUP_EVENTS = "send I X 1\nsend X Y 2\nsend Y I 3\nsend Z I 1\nsnapshot X\ntick 2\nsend X Z 1\nsnapshot I\n"

# X -> Y holds three tokens before any tick and X's marker after them: with two ring slots per
# channel every instance spills there
SPILL_EVENTS = "send X Y 1\nsend X Y 2\nsend X Y 1\nsnapshot X\ntick 2\nsend I Y 1\nsnapshot Y\n"

# K has no out-link; ten snapshots use both pending words of a node
SINK_TOP = "4\nA 9\nB 9\nM 9\nK 9\nA B\nB A\nA M\nM A\nB M\nM K\nA K\n"
TEN_SNAPSHOTS_EVENTS = "send A K 2\nsend M K 1\n" + "".join(
    f"snapshot {x}\ntick 1\nsend {x} {y} 1\n" for x, y in zip("ABMABMABMA", "MAKBMABAAK"))

# Two nodes, each starts a snapshot before the first tick: each snapshot's closing marker travels
# on the other node's link, and the two are delivered in the same tick wherever the delays agree,
# as in a row of equal delays.  The token ahead of A's marker makes A -> B a token link.
PAIR_TOP = "2\nA 5\nB 5\nA B\nB A\n"
SAME_TICK_EVENTS = "send A B 1\nsnapshot A\nsnapshot B\n"

# S has no in-link: a snapshot started there never completes, the drain ends in HANG
SOURCE_TOP = "4\nS 9\nA 9\nB 9\nK 9\nS A\nS B\nA B\nB A\nA K\nB K\n"
SOURCE_EVENTS = "send S A 1\nsnapshot S\ntick 1\nsnapshot A\nsend A B 1\n"

# (name, topology, events) of every program the host test compiles
COMPILE_CASES = [
    ("shared_cursor", T4_TOP, SHARED_CURSOR_EVENTS),
    ("degree4_mixed", STAR_TOP, STAR_EVENTS),
    ("no_send", T4_TOP, NO_SEND_EVENTS),
    ("every_channel", T4_TOP, EVERY_CHANNEL_EVENTS),
    ("insufficient", T4_TOP, INSUFFICIENT_EVENTS),
    ("unknown_dest", T4_TOP, UNKNOWN_DEST_EVENTS),
    ("send_group", T4_TOP, GROUP_EVENTS),
    ("spill", T4_TOP, SPILL_EVENTS),
    ("ten_snapshots", SINK_TOP, TEN_SNAPSHOTS_EVENTS),
    ("same_tick", PAIR_TOP, SAME_TICK_EVENTS),
    ("source_initiator", SOURCE_TOP, SOURCE_EVENTS),
]
