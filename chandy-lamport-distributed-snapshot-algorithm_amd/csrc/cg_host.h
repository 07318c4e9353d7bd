// cg_host.h -- what the graph readouts (cg_readout.cpp) and the restore (cg_restore_host.cpp) know
// of a cl_graph: cg_host.cpp defines the graph and the functions of the first part, cg_readout.cpp
// the second.  A readout and the restore read a graph through these only; they see no field of it.
#pragma once
#include "../../include/clgraph.h"
#include "cg_engine.h"
#include "cl_dev.h"

namespace clsnap {

// ---- of both units ------------------------------------------------------------------------------
// The opening of an ABI call on a graph: a null handle is refused (no lock: one thread drives a graph).
#define GRAPH_CALL(g) \
  if (!(g)) return clsnap::set_err(CL_E_INVALID, "null cl_graph handle")

// The return of a cg_launch_* call as an ABI code.
inline int launch_err(int e) {
  return e ? set_err(CL_E_DEVICE, "graph kernel launch failed: %s", hipGetErrorString((hipError_t)e)) : CL_OK;
}

// The timing events of a call (timing only: no cache writeback per record).
template <int N>
using GraphTimer = DevTimer<N, hipEventDisableSystemFence>;

// ---- of cg_host.cpp ---------------------------------------------------------------------------
// What the argument checks need; no device work behind it (every argument is checked before any).
struct GraphFacts {
  int32_t n_sids;
  bool part;                 // a partitioned run (cl_graph_part_begin)
  int32_t node_lo, node_hi;  // the owned nodes: all outside the partitioned mode, [0, 0) before the freeze
};
GraphFacts graph_facts(const cl_graph* g);

// 0 <= sid_lo <= sid_hi <= the snapshots started so far, or CL_E_INVALID.
int sid_range_ok(const cl_graph* g, int32_t sid_lo, int32_t sid_hi);

// The engine's state on the device, valid until the next event or setter of the graph.
struct GraphView {
  const GParams* P;
  hipStream_t stream;
  int32_t n_cus;           // the CU count the grids are sized by
  const int32_t* d_in_ch;  // [e] channel of every in-position (resident with the topology)
  int32_t k_lo, k_hi;      // the in-CSR range of the owned nodes
  int32_t hist;            // payload history slots per channel, 0: every message carries 1 token
};
// Executes what is pending, waits for it, and fills *out.
int graph_view(cl_graph* g, GraphView* out);

// out[sid - sid_lo] = rank of the initiator of sid in [sid_lo, sid_hi) (the program's snapshot events), -1 for none.
void graph_initiators(const cl_graph* g, int32_t sid_lo, int32_t sid_hi, long long* out);

// The seed of a restored graph (cl_graph_restore, cg_restore_host.cpp builds it; cg_engine.h GSeed
// draws the layout): the initial token plane, the entries and payloads on the device, what
// cl_graph_seed_info_of reports, and the timing of the build and of the latest seeding.
struct GraphSeed {
  cl_graph_seed_info info{};
  DevBuf<int32_t> init_tok;        // [n] the recorded node tokens
  DevBuf<int32_t> channel, count;  // [info.channels]
  DevBuf<long long> moff;          // [info.channels]
  DevBuf<int32_t> msgs;            // [info.msgs]; empty with unit payloads
  double build_ms = 0;
  GraphTimer<2> seed_t;            // around the seed kernel of the latest run from the initial state
  // a partitioned run begun from the seed (cl_graph_part_begin_seeded): this device's slice
  DevBuf<long long> d_share;       // [4] entry lo, entry hi, message lo, message hi
  int64_t share[4] = {0, 0, 0, 0};
  bool shared = false;
  int64_t device_bytes() const {
    return (int64_t)(init_tok.bytes() + channel.bytes() + count.bytes() + moff.bytes() + msgs.bytes() + d_share.bytes());
  }
};
// A new graph on g's device with g's frozen topology (host arrays copied, device arrays copied
// device to device) and g's limits, push lanes and delay source; no traffic, trace, program or
// bound stream.  g's topology is resident: g has run (graph_view succeeded), or
// graph_topology_resident has.
int graph_clone_frozen(const cl_graph* g, cl_graph** out);
// The topology of a graph that serves as a template only (cl_graph_restore_cut): it need never
// have had an event.  graph_topology freezes it like any call that needs rank order, on the
// host alone; graph_topology_resident makes g's device current, uploads the topology's arrays if
// they are not there yet, allocates none of g's run planes, and returns the stream to build on
// and the CU count.
struct GraphTopo {
  int32_t n;  // nodes
  int64_t e;  // channels
};
int graph_topology(cl_graph* g, GraphTopo* out);
int graph_topology_resident(cl_graph* g, hipStream_t* stream, int32_t* n_cus);
// Hands r its seed (r owns it from here on): r's runs start from it, its initial tokens are the
// seed's plane and its token total counts the seeded payloads.
void graph_adopt_seed(cl_graph* r, GraphSeed* seed);
GraphSeed* graph_seed(const cl_graph* g);  // nullptr: not made by restore

// ---- of cg_readout.cpp --------------------------------------------------------------------------
// A graph's readout scratch and timers; the graph makes it with itself and deletes it once its streams are idle.
struct Readouts;
Readouts* readouts_new();
void readouts_delete(Readouts* r);
Readouts* graph_readouts(const cl_graph* g);  // (defined in cg_host.cpp)
int64_t readouts_device_bytes(const Readouts* r);

}  // namespace clsnap
