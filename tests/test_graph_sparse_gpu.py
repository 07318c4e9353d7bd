"""GPU tests of the graph engine's sparse packed collect (GraphSim.collect_sparse,
cl_graph_collect_sparse) against the CPU oracle (sparsecheck.expected_sparse), the dense
collect and the summary table -- all exact.  Shapes: fewer channels than one wave (the
reference scenarios), several channel tiles with a ragged last one (2000-node power-law,
600-node regular), unit and non-unit payloads, complete and incomplete snapshots."""
import functools

import numpy as np
import pytest

import graphcheck as GC
import oracle as O
import sparsecheck as S
import tablecheck as T

pytestmark = pytest.mark.gpu

cl, clg = GC.cl, GC.clg


def check_dense(g, o, s, sid):
    """dense(sid) equals the oracle's channel CSR and the engine's dense collect."""
    e = g.num_channels
    tok, off, msg = s.dense(sid, e)
    for want in (o.collect_channels(sid), g.collect_arrays(sid)):
        for a, b in zip((tok, off, msg), want):
            assert a.dtype == b.dtype == np.int64
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("top,events,unit", [("2nodes.top", "2nodes-message.events", 1),
                                             ("8nodes.top", "8nodes-concurrent-snapshots.events", 0),
                                             ("10nodes.top", "10nodes.events", 0)])
def test_reference_scenarios(top, events, unit):
    """Fewer channels than one wave.  2nodes-message sends single tokens only (no payload
    history); the other two send several tokens at once, so their payloads come from the
    history."""
    g = GC.scenario_engine(top, events, O.REFERENCE_SEED)
    o = GC.scenario_oracle(top, events, O.REFERENCE_SEED)
    ns = o.num_snapshots
    assert g.status() == o.status == 0 and g.num_snapshots == ns and ns > 0
    s = g.collect_sparse(tokens=True)
    S.assert_sparse_equal(s, S.expected_sparse(o, 0, ns))
    assert s.complete.all() and s.n_msgs > 0
    rc, info = g._collect_sparse(0, ns)
    assert rc == cl.E_LIMIT and info["unit_payloads"] == unit
    assert (s.msg_tokens.max() > 1) == (not unit)
    for sid in range(ns):
        check_dense(g, o, s, sid)
        got, want = s.snapshot(sid, g), g.CollectSnapshot(sid)
        assert (got.id, got.tokenMap) == (want.id, want.tokenMap)
        assert [m.astuple() for m in got.messages] == [m.astuple() for m in want.messages]


@functools.lru_cache(maxsize=None)
def powerlaw_run():
    """(engine, oracle, expected full-range SparseSnapshots) of the drained power-law run: unit
    payloads, 12 snapshots over several channel tiles."""
    p, o, _ = T.powerlaw_drained()
    g = GC.engine_program(p, drain=True)
    assert g.status() == o.status == 0
    return g, o, S.expected_sparse(o, 0, o.num_snapshots)


def test_unit_payloads_over_several_tiles():
    g, o, want = powerlaw_run()
    ns = o.num_snapshots
    assert ns == 12 and g.num_channels > 4 * 2048 and g.num_channels % 2048 != 0
    full = g.collect_sparse(tokens=True)
    S.assert_sparse_equal(full, want)
    assert full.complete.all() and full.n_entries > 0 and (full.msg_tokens == 1).all()
    rc, info = g._collect_sparse(0, ns)
    assert rc == cl.E_LIMIT and info["unit_payloads"] == 1 and info["n_complete"] == ns
    assert (info["node_lo"], info["node_hi"]) == (0, g.num_nodes)
    S.assert_sparse_equal(g.collect_sparse(3, 7, tokens=True), S.expected_sparse(o, 3, 7))
    for sid in range(ns):
        S.assert_sparse_equal(g.collect_sparse(sid, sid + 1, tokens=True), S.expected_sparse(o, sid, sid + 1))
    bare = g.collect_sparse(payloads=False)
    S.assert_sparse_equal(bare, want, tokens=False)      # (unit payloads: all ones without a fetch)
    assert bare.tokens is None
    # the table's channel fields and digest, and the oracle's digest
    rows = g.snapshot_table().rows
    np.testing.assert_array_equal(np.diff(full.row_offsets), rows["rec_channels"])
    for sid in range(ns):
        a, b = full.msg_offsets[full.row_offsets[sid]], full.msg_offsets[full.row_offsets[sid + 1]]
        assert b - a == rows["rec_msgs"][sid]
        d = full.digest(sid, g.num_nodes, g.num_channels)
        assert d == rows["digest"][sid] == GC.digest_of(sid, *o.collect_channels(sid))
    for sid in (0, ns - 1):
        check_dense(g, o, full, sid)


def test_mixed_completion_and_poisoned_planes():
    p, o, _ = T.powerlaw_undrained()
    assert T.mixed(o)
    g = GC.engine_program(p)
    ns = o.num_snapshots
    want = S.expected_sparse(o, 0, ns)
    s = g.collect_sparse(tokens=True)
    S.assert_sparse_equal(s, want)
    done = np.array([o.complete(sid) for sid in range(ns)])
    assert done.any() and not done.all()
    np.testing.assert_array_equal(s.complete != 0, done)
    assert (np.diff(s.row_offsets)[~done] == 0).all() and (s.tokens[~done] == -1).all()
    assert (np.diff(s.row_offsets)[done] > 0).any() and (s.tokens[done] >= 0).all()
    with pytest.raises(cl.ClSnapError) as e:
        s.dense(int(np.nonzero(~done)[0][0]), g.num_channels)
    assert e.value.code == cl.E_NOT_COMPLETE
    # nothing comes from incomplete planes or stale buffers: poison, rerun, the same bytes
    g.poison_outputs()
    g.rerun()
    again = g.collect_sparse(tokens=True)
    for f in S.FIELDS:
        assert getattr(again, f).tobytes() == getattr(s, f).tobytes(), f


@functools.lru_cache(maxsize=None)
def regular_text_program():
    """A 600-node regular graph (about 4.8 k channels: more than two tiles, a ragged last one)
    driven through .top / .events text: send lines of 2 to 5 tokens on a few dozen channels
    around three snapshots, then readEventsFile's drain."""
    p = GC.regular_program(600, steps=1, seed=31)
    w = p.width()
    name = lambda r: f"N{int(r):0{w}d}"  # noqa: E731
    top = "\n".join([f"{p.n}"] + [f"{name(r)} {int(p.tokens[r])}" for r in range(p.n)] +
                    [f"{name(a)} {name(b)}" for a, b in zip(p.src, p.dst)]) + "\n"
    e = p.src.size
    ev = []
    for step in range(9):
        for j in range(36):                  # 36 channels spread over all tiles, revisited every step
            c = (j * 131 + (step % 3) * 7) % e
            ev.append(f"send {name(p.src[c])} {name(p.dst[c])} {2 + (j + step) % 4}")
        if step in (1, 3, 4):
            ev.append(f"snapshot {name((step * 197) % p.n)}")
        ev.append("tick")
    return p, top, "\n".join(ev) + "\n"


def test_nonunit_payloads_over_several_tiles():
    p, top, events = regular_text_program()
    o = O.OracleSim()
    o.use_counter_hash(p.delay_seed)
    assert o.read_topology_text(top) == 0
    assert o.read_events_text(events) == 0
    g = clg.GraphSim()
    g.read_topology_text(top)
    g.set_delay_hash(p.delay_seed)
    assert g.read_events_text(events) == 3
    g.flush()
    assert g.status() == o.status == 0
    e = g.num_channels
    assert 2 * 2048 < e < 3 * 2048
    s = g.collect_sparse(tokens=True)
    S.assert_sparse_equal(s, S.expected_sparse(o, 0, 3))
    assert s.complete.all() and s.n_entries > 0 and s.msg_tokens.max() > 1
    assert s.channel.min() < 2048 and s.channel.max() >= 2 * 2048      # entries in the first and the last tile
    rc, info = g._collect_sparse(0, 3)
    assert rc == cl.E_LIMIT and info["unit_payloads"] == 0
    bare = g.collect_sparse(payloads=False)
    S.assert_sparse_equal(bare, s, tokens=False, payloads=False)
    assert bare.msg_tokens is None
    rows = g.snapshot_table().rows
    for sid in range(3):
        check_dense(g, o, s, sid)
        assert s.digest(sid, g.num_nodes, e) == rows["digest"][sid]


def test_capacity_protocol():
    g, o, want = powerlaw_run()
    ns = o.num_snapshots
    ne, nm = want.n_entries, want.n_msgs
    assert ne > 1 and nm > 1
    complete = np.full(ns, -7, dtype=np.int32)
    offs = np.full(ns + 1, -7, dtype=np.int64)
    rc, info = g._collect_sparse(0, ns, complete, offs)                 # the sizing call
    assert rc == cl.E_LIMIT
    assert (info["n_sids"], info["n_complete"], info["n_entries"], info["n_msgs"]) == (ns, ns, ne, nm)
    np.testing.assert_array_equal(offs, want.row_offsets)
    np.testing.assert_array_equal(complete, want.complete)

    def fetch(ent_cap, msg_cap):
        ch = np.full(ne + 1, -7, dtype=np.int32)
        cn = np.full(ne + 1, -7, dtype=np.int32)
        msg = np.full(nm + 1, -7, dtype=np.int32)
        tok = np.full((ns, g.num_nodes), -7, dtype=np.int32)
        rc, info = g._collect_sparse(0, ns, None, None, ch, cn, ent_cap, msg, msg_cap, tok)
        assert (info["n_entries"], info["n_msgs"]) == (ne, nm)
        return rc, ch, cn, msg, tok

    rc, ch, cn, msg, tok = fetch(ne, nm)                                # exact caps
    assert rc == 0
    np.testing.assert_array_equal(ch[:ne], want.channel)
    np.testing.assert_array_equal(cn[:ne], want.count)
    np.testing.assert_array_equal(msg[:nm], want.msg_tokens)
    np.testing.assert_array_equal(tok, want.tokens)
    assert ch[ne] == cn[ne] == msg[nm] == -7                            # nothing past the totals
    for ent_cap, msg_cap in ((ne - 1, nm), (ne, nm - 1)):
        rc, ch, cn, msg, tok = fetch(ent_cap, msg_cap)
        assert rc == cl.E_LIMIT
        assert (ch == -7).all() and (cn == -7).all() and (msg == -7).all() and (tok == -7).all()


def test_sparse_time():
    p, _, _ = T.powerlaw_drained()
    g = GC.engine_program(p, drain=True)
    with pytest.raises(cl.ClSnapError) as e:
        g.sparse_time()
    assert e.value.code == cl.E_STATE
    g.collect_sparse(tokens=True)
    assert g.sparse_time() > 0
