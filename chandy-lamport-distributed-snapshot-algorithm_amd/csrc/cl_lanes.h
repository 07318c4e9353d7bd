// cl_lanes.h -- the batch engine's instance-per-lane kernel, specialized on the topology.
//
// cl_exec_kernel (cl_kernels.hip) lays an instance of N nodes across N lanes: every wave
// instruction serves 64 / N instances, lanes exchange pick words and draw offsets, and most
// per-node work runs predicated on lanes with nothing to deliver (BASELINE config 3: ~2.4 of
// an instance's 8 lanes deliver in an average tick).  This kernel runs ONE instance per lane,
// 64 per wave.  Every instance of a batch has the same topology (the reference's .top file),
// so the topology is compiled into the kernel: cl_jit.cpp generates a topology type T (node
// count, degrees, CSR offsets, in-link senders) for the frozen topology and compiles this header
// with hipRTC for gfx950 at run time.  Every loop over node slots v < N and link slots is then
// unrolled with constant bounds and constant channel numbers: a node's state lives in
// registers of a fixed slot -- tokens, out-link head words, in-link recording cursors,
// per-snapshot pending nibbles -- and a sender's pick word reaches its receivers as a register
// read.  Only data-dependent addresses go through the lane's private LDS column (word k at
// lds[k * 64 + lane], conflict-free for any per-lane index): the FIFO rings (a head or tail
// slot differs per lane) and the instance's delay row.
//
// One tick (sim.go:71-95), exact in the reference's order:
//   A pick     every sender scans its out-links in dest order and pops the first due head;
//              picks from tick-start state are exact (a push made in tick t is due at >= t+1
//              and never changes a non-empty queue's head).
//   B receive  every receiver walks its in-links in ascending sender rank (the in-CSR order)
//              and handles the packet its sender picked for it: token -> tokens += n,
//              cursor++; marker -> CreateLocalSnapshot / close the channel (node.go:149-185).
//   C offsets  first-receipt markers broadcast (node.go:97-109) drawing their delays in
//              triggering-sender order: the exclusive prefix of the broadcasts' out-degrees
//              over senders.
//   D push     each receiver pushes its broadcasts on its out-links.
// Snapshot completion (sim.go:126-131) is one check per tick over the pending nibbles.
// Outputs, state image, spill rings and the replay plan are the node-parallel kernel's
// (cl_engine.h), so either kernel continues the other's launches.
// Reference map (paths relative to /root/reference/chandy_lamport): Tick sim.go:71-95,
// GetReceiveTime sim.go:100-102, StartSnapshot sim.go:105-123, NotifyCompletedSnapshot
// sim.go:126-131, CreateLocalSnapshot node.go:58-84, SendToNeighbors node.go:97-109,
// SendTokens node.go:112-131, HandleMarker node.go:149-171, HandleToken node.go:174-185,
// drain test_common.go:123-137.
//
// The topology type T provides (all constexpr):
//   N, D, SW             nodes, degree bound (every in- and out-degree <= D), pending words
//                        per node (8 snapshot ids each)
//   id(v), od(v)         in- and out-degree of node v
//   off(v)               first channel of node v (channels by (src rank, dest rank))
//   E, CAPL              channels, log2 of the LDS ring slots per channel
//   PCAPL                log2 of the ring slots of the launch's layout: below CAPL on the
//                        deep-ring kernel, which flags pushes past that ring in a probe
//   BLK                  snapshot records block-major by launch slot (cl_engine.h rec_word)
//   src(v, j), oix(v, j) in-link j of node v: sender rank and the link's out-index there
//   dst(v, k), ipos(v, k) out-link k of node v: receiver rank and the link's in-index there
#pragma once
#include "cl_engine.h"

namespace clsnap {
namespace lanes {

typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef const __attribute__((address_space(4))) ExecParams KPar;

// The kernel's parameters re-read from the kernarg segment (ExecParams is the first argument,
// at offset 0).  The empty asm makes every load through the pointer a fresh scalar load at its
// point of use instead of a value the compiler hoists out of the tick loop and keeps live.
__device__ __forceinline__ KPar* kpar() {
  auto* k = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return (KPar*)k;
}

// Words per node snapshot record for degree bound D (rec_words of an unrolled layout).
constexpr int rec_w(int D) { return D == 1 ? 2 : D <= 3 ? 4 : 8; }

// Per-lane constants.
// LDS layout, per lane a private column:
//   FIFO rings, 16-bit entries: channel c's slot q is element (c << CAPL) + q, element i of
//   lane l at byte i * 128 + l * 2 (FW = E << CAPL >> 1 words of 256 bytes in all)
//   then 32-bit words, word w of lane l at byte w * 256 + l * 4:
//     FW            scratch word (stores that do not happen land here)
//     FW + 1 ..     the delay row, 8 nibbles per word (reads clamped to its last word: a
//                   read past the end only feeds pushes past `draws`, which fail anyway)
//     then          one pad word (never written: the second word of a read at the row's end)
// A 16-bit FIFO entry: bits 7..0 receiveTime mod 256, bits 14..8 payload (token count or
// snapshot id, < 128), bit 15 marker.  receiveTime is recovered from its low byte because an
// entry is never more than draws + 4 ticks late when it is examined: while it is due but not
// delivered, either its queue's head is not yet due -- at most 4 ticks, as every packet behind
// a head was pushed no earlier and draws a delay of at most 4 -- or the sender delivers another
// packet that tick, and an instance delivers at most as many packets as it pushes (one draw
// each).  The host admits a program only with draws <= 240 (cl_jit.cpp lanes_fit), and an
// entry is due when (time - receiveTime) mod 256 < 251.
struct Ctx {
  uint32_t lb;      // this lane's byte offset in the 32-bit words: lane * 4
  uint32_t lb2;     // ... in the 16-bit FIFO elements: (lane & 31) * 4 + (lane >> 5) * 2
  uint32_t inst;    // instance of this lane (0 for lanes without one)
  uint32_t stride;
  uint32_t lrec;    // byte offset of this instance's node records in snapshot plane 0
  uint32_t plane8;  // bytes per snapshot plane / 256 (the stride is a multiple of 64)
  int32_t draws;    // delays per instance
  uint32_t dlast;   // column word of the delay row's last word
};

__device__ __forceinline__ lds_u32* lds_at(uint32_t byte) { return (lds_u32*)(size_t)byte; }
typedef __attribute__((address_space(3))) uint16_t lds_u16;
__device__ __forceinline__ lds_u16* lds16_at(uint32_t byte) { return (lds_u16*)(size_t)byte; }
// FIFO element i of this lane (cold paths: prologue, epilogue)
struct Ctx;
__device__ __forceinline__ uint32_t fifo_rd(const Ctx& x, uint32_t i);
__device__ __forceinline__ void fifo_wr(const Ctx& x, uint32_t i, uint32_t v);
__device__ __forceinline__ uint32_t fifo_rd(const Ctx& x, uint32_t i) { return *lds16_at(x.lb2 + (i << 7)); }
__device__ __forceinline__ void fifo_wr(const Ctx& x, uint32_t i, uint32_t v) { *lds16_at(x.lb2 + (i << 7)) = (uint16_t)v; }
__device__ __forceinline__ uint32_t col_rd(const Ctx& x, uint32_t w) { return *lds_at(x.lb + (w << 8)); }
__device__ __forceinline__ void col_wr(const Ctx& x, uint32_t w, uint32_t v) { *lds_at(x.lb + (w << 8)) = v; }

template <class T>
struct Lds {
  static constexpr uint32_t CAP = 1u << T::CAPL;
  static constexpr uint32_t CAPM7 = (CAP - 1u) << 7;  // a head word's ring-slot byte offset bits
  static constexpr uint32_t FW = ((uint32_t)T::E << T::CAPL) / 2;
  static constexpr uint32_t DUMMY = FW, DB = FW + 1;
};
// receiveTime <= time for a 16-bit entry (see the layout note): 1 or 0
__device__ __forceinline__ uint32_t due16(uint32_t e, int32_t time) {
  return (((((uint32_t)time - e) & 0xffu)) - 251u) >> 31;
}
// Two 16-bit values in the halves of a register, for the packed 16-bit VALU (v_pk_*_u16).
typedef uint16_t us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ us2 as_us2(uint32_t v) { return __builtin_bit_cast(us2, v); }
__device__ __forceinline__ uint32_t as_u32(us2 v) { return __builtin_bit_cast(uint32_t, v); }
// due16 of two entries against the time's low 16 bits in both halves of t2: 1 or 0 per half
__device__ __forceinline__ uint32_t due16x2(uint32_t e2, us2 t2) {
  const us2 d = as_us2(as_u32(t2 - as_us2(e2)) & 0x00ff00ffu) - (us2)(251);
  return as_u32(d >> (us2)(15));
}
// min(half, 1) per half: a count's non-empty flag in one instruction (the compiler takes a min
// on a 16-bit pair apart into compares, selects and a v_perm_b32)
__device__ __forceinline__ uint32_t pk_min1(uint32_t c2) {
  uint32_t r;
  asm("v_pk_min_u16 %0, %1, 1 op_sel_hi:[1,0]" : "=v"(r) : "v"(c2));
  return r;
}
// the node-parallel kernel's 32-bit entry (state image, HBM spill rings) and back
__device__ __forceinline__ uint32_t e16_to_32(uint32_t e, int32_t time) {
  const uint32_t rt = (uint32_t)time + 5u - (((uint32_t)time + 5u - e) & 0xffu);
  return ((e & 0x8000u) << 16) | ((e >> 8) & 0x7fu) | (rt << 16);
}
__device__ __forceinline__ uint32_t e32_to_16(uint32_t e) {
  return ((e >> 16) & 0xffu) | ((e & 0x7fu) << 8) | ((e >> 16) & 0x8000u);
}

// Delays k .. k + 7 of this instance as 4-bit nibbles (two column words, one ds_read2st64).
template <class T>
__device__ __forceinline__ uint32_t delays8(const Ctx& x, int32_t k) {
  // (w + 1 is at most the pad word after the row: one ds_read2st64 with a single clamp; C3 1.553 ->
  // 1.541 ms per step, gpurun_out/r06ab7)
  const uint32_t w = min(Lds<T>::DB + ((uint32_t)k >> 3), x.dlast);  // (k >= 0)
  const uint32_t lo = col_rd(x, w), hi = col_rd(x, w + 1);
  return __builtin_amdgcn_alignbit(hi, lo, ((uint32_t)k & 7u) * 4u);
}

// Byte offset of node v's record from an instance's first record in one plane: instance-major
// (an instance's N records contiguous), or block-major by launch slot (T::BLK: the wave's 64
// records of node v contiguous, cl_engine.h rec_word)
template <class T>
__device__ __forceinline__ uint32_t node_off(const Ctx& x, uint32_t v) {
  (void)x;
  return v * (uint32_t)(rec_w(T::D) * 4 * (T::BLK ? 64 : 1));
}

// Byte offset of snapshot plane `sid` on the full-rate 24-bit multiplier (cl_kernels.hip plane_off).
// (No asm barrier on the product here, unlike the node-parallel kernel: the compiler keeps the
// 24-bit multiply, and the barrier's register copy in each in-link's record address cost 6 VGPR
// spills around the tick loop; C3 1.544 -> 1.496 ms per step, gpurun_out/r06ab8.)
__device__ __forceinline__ uint32_t plane_off(const Ctx& x, uint32_t sid) {
  return __umul24(sid, x.plane8) << 8;
}

template <class V>
__device__ __forceinline__ void st_at(V* base, uint32_t byte_off, V val) {
  *reinterpret_cast<V*>(reinterpret_cast<char*>(base) + byte_off) = val;
}

// The instruction scheduler may not move anything across this point: it keeps the unrolled
// node slots from being interleaved into one long region where every slot's lane masks are
// live at once (SGPR spills to VGPR lanes).
__device__ __forceinline__ void sched_fence() { __builtin_amdgcn_sched_barrier(0); }

// A value the optimizer cannot see through (op dispatch below).
template <class V>
__device__ __forceinline__ V opaque(V v) {
  asm volatile("" : "+v"(v));
  return v;
}

// Diagnostic build (dbg library, CLSNAP_TIMELINE=1; never the product): where a wave's shader
// clock cycles go, by segment of program().  mark(k) adds the cycles since the previous stamp
// to segment k (s_memtime: a scalar read, the same value for the whole wave); drain() waits for
// every vector memory operation the wave has in flight -- stores included, they share vmcnt
// with loads -- so the segment marked after it is the time the wave would spend parked at its
// next use of a loaded value (after a tick loop: the reloads of the registers spilled around
// it, which queue behind the loop's record stores).  Lane 0 adds the wave's segments to
// clsnap_lanes_tl[kernel][block & 63] (64 copies: no contended word), read and summed by
// cl_lanes_timeline_read (cl_jit.cpp).
enum { TL_ROW, TL_PRO, TL_OPS, TL_LOOP, TL_WAIT, TL_EPI, TL_WAVES, TL_LOOPS, TL_NUM };
#if defined(CLSNAP_TIMELINE)
extern "C" {
__device__ unsigned long long clsnap_lanes_tl[2][64][TL_NUM];
}
struct Timeline {
  uint64_t last;
  uint32_t seg[TL_NUM];
  __device__ __forceinline__ static uint64_t now() {
    __builtin_amdgcn_sched_barrier(0);
    const uint64_t t = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
    return t;
  }
  __device__ __forceinline__ void begin() {
#pragma unroll
    for (int k = 0; k < TL_NUM; ++k) seg[k] = 0;
    seg[TL_WAVES] = 1;
    last = now();
  }
  __device__ __forceinline__ void mark(int k) {
    const uint64_t t = now();
    seg[k] += (uint32_t)(t - last);
    last = t;
  }
  __device__ __forceinline__ void count(int k) { seg[k] += 1; }
  __device__ __forceinline__ void drain() { __builtin_amdgcn_s_waitcnt(0x0f70); }  // vmcnt(0)
  __device__ __forceinline__ void flush(int kernel) {
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < TL_NUM; ++k)
        atomicAdd(&clsnap_lanes_tl[kernel][blockIdx.x & 63u][k], (unsigned long long)seg[k]);
    }
  }
};
#else
struct Timeline {
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void mark(int) {}
  __device__ __forceinline__ void count(int) {}
  __device__ __forceinline__ void drain() {}
  __device__ __forceinline__ void flush(int) {}
};
#endif

// Compile-time loop: f(IC<I>) for I in [B, E).
template <int I>
struct IC {
  static constexpr int value = I;
};
template <int B, int E, class F>
__device__ __forceinline__ void sfor(F&& f) {
  if constexpr (B < E) {
    f(IC<B>{});
    sfor<B + 1, E>(f);
  }
}

// Senders in pairs.  Everything phase A does to an out-link works on 16-bit data -- a FIFO entry,
// a head word, 0/1 flags -- and gfx950 runs packed 16-bit integer VALU at full rate, so two senders
// share every instruction of the scan: the low halves of the registers are one sender's, the
// high halves the other's.  The senders are sorted by out-degree (descending, ties by rank) and
// neighbours paired, so a pair's degrees differ as little as possible; with an odd N the last
// sender's partner half is inert, and so is the half of a link slot past its sender's out-degree:
// its head half stays 0 (never non-empty, so never looked at, due or popped) and its entry half
// is 0.
template <class T>
struct Pairs {
  static constexpr int NP = (T::N + 1) / 2;
  struct Tab {
    int snd[NP][2];  // pair p's senders: low half, high half (-1: inert)
    int pr[T::N], hf[T::N];
  };
  static constexpr Tab make() {
    Tab t{};
    int ord[T::N] = {};
    for (int v = 0; v < T::N; ++v) {  // insertion sort, stable
      int i = v;
      for (; i > 0 && T::od(ord[i - 1]) < T::od(v); --i) ord[i] = ord[i - 1];
      ord[i] = v;
    }
    for (int p = 0; p < NP; ++p)
      for (int h = 0; h < 2; ++h) {
        const int v = 2 * p + h < T::N ? ord[2 * p + h] : -1;
        t.snd[p][h] = v;
        if (v >= 0) {
          t.pr[v] = p;
          t.hf[v] = h;
        }
      }
    return t;
  }
  static constexpr Tab tab = make();
  static constexpr int snd(int p, int h) { return tab.snd[p][h]; }
  static constexpr int pr(int v) { return tab.pr[v]; }         // node v's pair
  static constexpr uint32_t sh(int v) { return 16u * (uint32_t)tab.hf[v]; }  // ... and its half's shift
  static constexpr int od(int p, int h) { return tab.snd[p][h] < 0 ? 0 : T::od(tab.snd[p][h]); }
  static constexpr int nk(int p) { return od(p, 0) > od(p, 1) ? od(p, 0) : od(p, 1); }  // link slots
  // the halves of pair p's link slot k that hold a link: 1 per half
  static constexpr uint32_t present(int p, int k) { return (k < od(p, 0) ? 1u : 0u) | (k < od(p, 1) ? 0x10000u : 0u); }
};

// The generic kernels' program type: the program is read from `ops` (the program types that
// cl_jit.cpp generates are described with send_c / snap_c below).
struct NoProg {
  static constexpr bool SPEC = false;
  static constexpr bool COVER = false;
};

// The in-links that can carry a token.  A program-specialized kernel starts from the initial
// state and runs exactly the program P, so a token only ever travels on a channel that one of
// P's OP_SEND host ops names: on(v, j) for in-link j of node v is true when some send has
// a == src(v, j) and b == oix(v, j).  A send counts wherever it stands (the arm after the last
// tick op included) and whether or not it succeeds at run time; one with an unknown destination
// (b < 0) names no channel.  Every other in-link delivers markers only: phase B has no token
// path there, and its recording cursor is the constant 0.  Nor does it store an end cursor when
// its marker closes the channel: the store's value would be the constant 0, and the record holds
// that 0 already.  The kernel starts from the initial state (program(): P::SPEC || p.fresh), so
// a node's pending nibble for a snapshot id is non-zero only after this lane ran create_record
// for (node, sid) earlier in this same launch, and create_record writes the whole record in one
// vector store: c = 0 on a token-free in-link, c | c << 16 = 0 where the marker arrived on it.
// That holds on planes nobody zeroed, and only here: a kernel that can resume from a state image
// may close a record that an earlier launch created.  NoProg: true everywhere.
template <class T, class P>
struct TokIn {
  struct Tab {
    bool t[T::N][T::D];
  };
  static constexpr Tab make() {
    Tab t{};
    if constexpr (P::SPEC) {
      for (int h = 0; h < P::h0(P::NARM); ++h)
        if (P::hk(h) == OP_SEND && P::hb(h) >= 0) t.t[T::dst(P::ha(h), P::hb(h))][T::ipos(P::ha(h), P::hb(h))] = true;
    } else {
      for (int v = 0; v < T::N; ++v)
        for (int j = 0; j < T::D; ++j) t.t[v][j] = true;
    }
    return t;
  }
  static constexpr Tab tab = make();
  static constexpr bool on(int v, int j) { return tab.t[v][j]; }
};

// State of one instance.
//   hw[p][k]  link slot k of sender pair p (Pairs): the low half is the first sender's out-link
//             k, the high half the second's.  Per half: bits 6..0 queued packets (LDS ring + HBM
//             spill; the host admits a program only when no channel ever carries more than 127
//             packets), bits 15..7 the ring head as a free-running 9-bit counter (the ring sizes
//             divide 512, so half & CAPM7 = the head slot * 128 across a wrap).  Pop is + 0x7f per
//             half, push + 1 per half; the pop is a packed add, so a wrapping head counter does
//             not carry into the high half's count
//   cr[v][.]  in-link j's recording cursor (token packets delivered on the channel): u16 j & 1
//             of word j >> 1
//   pd[v][w]  per snapshot sid (w = sid >> 3) a nibble at 4 * (sid & 7): 0 not started,
//             pending + 1 after the node's local snapshot exists (1 = complete), 15 an initiator
//             without in-links (pending 0, but completion is only checked on a marker: never)
//   done[w]   bit 4 * (sid & 7) + 3 set once the instance's snapshot sid completed
template <class T>
struct State {
  int32_t tok[T::N];
  uint32_t hw[Pairs<T>::NP][T::D];
  uint32_t cr[T::N][(T::D + 1) / 2];
  uint32_t pd[T::N][T::SW];
  uint32_t done[T::SW];
  int32_t time, draw, status, flag;
  uint32_t peek, push, ndone;
  bool alive;
};

// out-link k of node v: its 16-bit head word
template <class T>
__device__ __forceinline__ uint32_t hw_get(const State<T>& s, int v, int k) {
  return (s.hw[Pairs<T>::pr(v)][k] >> Pairs<T>::sh(v)) & 0xffffu;
}
template <class T>
__device__ __forceinline__ uint32_t cur_get(const State<T>& s, int v, int j) {
  return (s.cr[v][j >> 1] >> ((j & 1) * 16)) & 0xffffu;
}

// pending nibble word of a per-lane snapshot id (SW = 2: a select between the two words)
template <class T>
__device__ __forceinline__ uint32_t pd_get(const State<T>& s, int v, uint32_t sid) {
  if constexpr (T::SW == 1) return s.pd[v][0];
  else return (sid & 8u) ? s.pd[v][1] : s.pd[v][0];
}
template <class T>
__device__ __forceinline__ void pd_set(State<T>& s, int v, uint32_t sid, uint32_t w) {
  if constexpr (T::SW == 1) {
    s.pd[v][0] = w;
  } else {
    const bool hi = (sid & 8u) != 0;
    s.pd[v][1] = hi ? w : s.pd[v][1];
    s.pd[v][0] = hi ? s.pd[v][0] : w;
  }
}

// Queue.Push (queue.go:18-20) on channel ch (ring at column word ring) with receiveTime =
// time + 1 + delay (sim.go:101), draw index kd.  Straight-line: the entry goes to its ring slot
// or, when the push does not land in the ring, to the lane's scratch word.  SPILL: a full LDS
// ring spills to the HBM ring under a rare branch.  Failures follow the node-parallel kernel:
// delay exhaustion, then overflow; the node's last failing push sets nf.
// hw is the pair's register and sh the channel's half (0 or 16; a caller that extracted the half
// passes 0): the low half needs no extraction, bits 15..7 of h + (h << 7) depend on it alone.
template <class T, bool SPILL>
__device__ __forceinline__ void push(const Ctx& x, uint32_t& hw, uint32_t sh, uint32_t ch, bool on, uint32_t pl16,
                                     int32_t kd, uint32_t delay, int32_t time, int32_t& nf) {
  using Ld = Lds<T>;
  static_assert(T::CAPL <= 9, "a ring's head slot must fit the half's 9-bit head counter");
  const uint32_t h = hw >> sh;
  const uint32_t cnt = h & 0x7fu;
  const bool dly_ok = kd < x.draws;
  const bool live = on && dly_ok;
  bool ok = live && cnt < Ld::CAP;
  const uint32_t rt = (uint32_t)(time + 1 + (int32_t)delay);
  const uint32_t e = pl16 | (rt & 0xffu);
  // the ring slot (head + count) mod ring slots, its byte address, or the scratch word
  const uint32_t slot = (x.lb2 | ((h + (h << 7)) & Ld::CAPM7)) + (ch << (T::CAPL + 7));
  *lds16_at(ok ? slot : x.lb + (Ld::DUMMY << 8)) = (uint16_t)e;
  if constexpr (SPILL) {
    if (__builtin_expect(live && cnt >= Ld::CAP, 0)) {  // LDS ring full: the HBM spill ring
      KPar* p = kpar();
      const int32_t ocap = p->lay.ocap_log2;
      if (ocap >= 0 && cnt - Ld::CAP < (1u << ocap)) {
        const uint32_t om = (1u << ocap) - 1;
        uint32_t* hp = &p->ovh[ch * x.stride + x.inst];
        uint32_t h = 0;
        if (cnt == Ld::CAP) *hp = 0u;  // nothing spilled yet: the ring restarts at slot 0
        else h = *hp;
        p->ovf[((ch << ocap) + ((h + cnt - Ld::CAP) & om)) * x.stride + x.inst] =
            ((pl16 & 0x8000u) << 16) | ((pl16 >> 8) & 0x7fu) | (rt << 16);  // (the 32-bit entry)
        if (p->spill_flag) p->spill_flag[x.inst] = 1;
        ok = true;
      }
    }
  }
  if constexpr (!SPILL && T::PCAPL < T::CAPL) {
    // the deep-ring kernel's probe: a push landing past the layout's ring flags its instance
    // as one that spills there (cl_host.cpp build_plan); replays pass no flag array
    if (__builtin_expect(ok && cnt >= (1u << T::PCAPL), 0)) {
      KPar* p = kpar();
      if (p->spill_flag) p->spill_flag[x.inst] = 1;
    }
  }
  hw += ok ? 1u << sh : 0u;  // (the push count is derived at the epilogue: pops + packets still queued)
  nf = (on && !ok) ? (dly_ok ? (int32_t)ST_FIFO_OVERFLOW : (int32_t)ST_DELAY_EXHAUSTED) : nf;
}

// The guard of a broadcast's fast path.  push() asks two questions per link that are false for
// almost every trigger: does the row still hold this draw, and is the ring full.  Both can be
// asked once per trigger: is the broadcast's last draw past the row (k0 + od > draws), and does
// the OR of the node's out-link head words have a bit of FULL, the count bits at or above the
// ring's slots (a power of two: some count >= CAP), masked to the node's own half of its pair's
// registers.  On the deep-ring kernel the bound is the
// layout's ring, so the probe's flag store stays in push().
// A program type with COVER set was compiled for a launch whose rows hold at least the program's
// own bound on draws (the host's draws_needed: one per send, one per snapshot id and channel), so
// no broadcast of an instance can run past its row and the first question is not asked at all.
// That concerns tick()'s first pass and snap_c only: push() on the slow path and in the further
// passes keeps its own row test, and start_snapshot, which only the generic kernels run, asks
// both questions as before.
template <class T>
struct Guard {
  static constexpr uint32_t LIM = 1u << (T::PCAPL < T::CAPL ? T::PCAPL : T::CAPL);
  static constexpr uint32_t FULL = 0x7fu & ~(LIM - 1u);
};

// The push that cannot fail (the guard held for every lane of the wave whose trigger is on), in
// its two parts: the ring slot's per-lane address bits from the head word, and the entry.  No
// draw or ring test, no status.  The callers store under the trigger's lane mask, so a lane whose
// trigger is off stores nothing (a select against the scratch word per link, as push() has it,
// compiled to 44 more VALU in the tick and 168 VGPRs), with the channel's constant
// ch << (CAPL + 7) in the DS instruction's immediate offset as in phase A's read, and add the
// trigger as a 0/1 integer to the head word's half.  (sh as in push(): one shift for a high half.)
template <class T>
__device__ __forceinline__ uint32_t sure_slot(const Ctx& x, uint32_t hw, uint32_t sh) {
  const uint32_t h = hw >> sh;
  return x.lb2 | ((h + (h << 7)) & Lds<T>::CAPM7);
}
__device__ __forceinline__ uint32_t sure_entry(uint32_t pl16, uint32_t delay, int32_t time) {
  return pl16 | ((uint32_t)(time + 1 + (int32_t)delay) & 0xffu);
}

// CreateLocalSnapshot (node.go:58-84) at node v: record tokens and open every in-channel except
// the one the first marker arrived on (arrive = -1 at the initiator): one vector store.  An
// in-link that carries no token under P (TokIn) records the constant 0.
template <class T, class P>
__device__ __forceinline__ void create_record(const Ctx& x, uint32_t* snod, const State<T>& s, int v, int arrive,
                                              uint32_t rb) {
  constexpr int RW = rec_w(T::D);
  uint32_t r[RW];
  r[0] = (uint32_t)s.tok[v];
#pragma unroll
  for (int j = 0; j < RW - 1; ++j) {
    const bool tl = j < T::D && j < T::id(v) && TokIn<T, P>::on(v, j < T::D ? j : 0);
    const uint32_t c = tl ? cur_get(s, v, j < T::D ? j : 0) : 0u;
    r[1 + j] = j == arrive ? (c | (c << 16)) : c;
  }
  const uint32_t o = rb + node_off<T>(x, (uint32_t)v);
#if defined(CLSNAP_ABL_NOSTORE)
  if (o != 0xffffffffu) return;  // (timing ablation: no record stores)
#endif
  if constexpr (RW == 2) {
    st_at(reinterpret_cast<uint2*>(snod), o, make_uint2(r[0], r[1]));
  } else {
#pragma unroll
    for (int q = 0; q < RW; q += 4)
      st_at(reinterpret_cast<uint4*>(snod), o + 4u * q, make_uint4(r[q], r[q + 1], r[q + 2], r[q + 3]));
  }
}

// Fold the lane's engine failure into its status (the instance freezes after the step).
template <class T>
__device__ __forceinline__ void resolve(State<T>& s) {
  if (s.flag != 0 && s.alive) {
    s.status = s.flag;
    s.alive = false;
  }
  s.flag = 0;
}

// Tick (sim.go:71-95) for a lane whose instance is `act`.  Every lane of the wave calls it.
// Returns true when no lane of the wave picked a packet (the tick ended after phase A).
// P: the program the kernel is specialized on (phase B's token path exists only on the in-links
// of TokIn<T, P>).
template <class T, bool SPILL, class P>
__device__ __forceinline__ bool tick(const Ctx& x, State<T>& s, bool act) {
  constexpr int N = T::N, D = T::D;
  s.time += act ? 1 : 0;
  // ---- A: pick, two senders per instruction (Pairs) ---------------------------------------
  // every head first (independent LDS reads: a pair's two entries into the halves of one
  // register), then the scan
  using Pr = Pairs<T>;
  constexpr int NP = Pr::NP;
  uint32_t e[NP][D];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int k = 0; k < D; ++k) {
      if (k >= Pr::nk(p)) continue;
      const uint32_t w = s.hw[p][k];
      us2 ev = (us2)(0);
      if (k < Pr::od(p, 0)) ev.x = lds16_at(x.lb2 | (w & Lds<T>::CAPM7))[(T::off(Pr::snd(p, 0)) + k) << (T::CAPL + 6)];
      if (k < Pr::od(p, 1))
        ev.y = lds16_at(x.lb2 | ((w >> 16) & Lds<T>::CAPM7))[(T::off(Pr::snd(p, 1)) + k) << (T::CAPL + 6)];
      e[p][k] = as_u32(ev);
    }
  uint32_t pk[N];  // sender v's pick: (out-index + 1) << 16 | the 16-bit entry (0: nothing)
  uint32_t es[N];  // sender v's out-links that were empty when it scanned them: their number
  // Peek (sim.go:83) counts of the tick, per half.  A tick adds at most D per pair and half,
  // NP * D <= 64 * 128 in all (cl_jit.cpp lanes_fit bounds N and D far below), so a half cannot
  // overflow before the fold below.
  uint32_t peek2 = 0;
  uint32_t any = 0;
  const us2 t2 = (us2)((uint16_t)s.time);
  // 0/1 integers per half in VGPRs, kept opaque: as compare masks the compiler would keep every
  // channel's masks live in SGPR pairs across the phase (and spill them to VGPR lanes)
  const uint32_t sc0 = opaque(act ? 0x10001u : 0u);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    uint32_t pke = 0, pki = 0;  // the halves' picked entries, and their out-index + 1
    uint32_t lks = 0, scs = 0;  // links looked at; links scanned (still scanning when reached)
    uint32_t sc = sc0;          // still scanning
#pragma unroll
    for (int k = 0; k < D; ++k) {
      if (k >= Pr::nk(p)) continue;
      const uint32_t w = s.hw[p][k];
      const uint32_t ne = pk_min1(w & 0x007f007fu);      // queue non-empty
      const uint32_t le = opaque(due16x2(e[p][k], t2));  // receiveTime <= time
      const uint32_t lk = sc & ne;                       // Peek (sim.go:83)
      lks += lk;  // (plain adds and subtracts where no half can carry or borrow)
      scs += Pr::present(p, k) == 0x10001u ? sc : sc & Pr::present(p, k);
      const uint32_t due = opaque(lk & le);
      if constexpr (SPILL) {
        // a due head whose queue reaches past the LDS ring (some half's count >= CAP, then
        // exactly per half): refill the freed slot from the spill ring
        if (__builtin_expect(due != 0 && (w & ((0x7fu & ~(Lds<T>::CAP - 1u)) * 0x10001u)) != 0, 0)) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if (k >= Pr::od(p, h)) continue;
            const uint32_t wh = w >> (16 * h);
            if (((due >> (16 * h)) & 1u) && (wh & 0x7fu) > Lds<T>::CAP) {
              KPar* kp = kpar();
              const uint32_t c = T::off(Pr::snd(p, h)) + k;
              const int32_t ocap = kp->lay.ocap_log2;
              uint32_t* hp = &kp->ovh[c * x.stride + x.inst];
              const uint32_t hd = *hp;
              lds16_at(x.lb2 | (wh & Lds<T>::CAPM7))[c << (T::CAPL + 6)] =
                  (uint16_t)e32_to_16(kp->ovf[((c << ocap) + hd) * x.stride + x.inst]);
              *hp = (hd + 1) & ((1u << ocap) - 1);
            }
          }
        }
      }
      // Pop: per half head + 1, count - 1 (one packed multiply-add)
      s.hw[p][k] = as_u32(as_us2(due) * (us2)(0x7f) + as_us2(w));
      // a half is due at most once in its scan (it stops scanning), so the pick accumulates
      pke = as_u32(as_us2(e[p][k]) * as_us2(due) + as_us2(pke));
      pki = as_u32(as_us2(due) * (us2)((uint16_t)(k + 1)) + as_us2(pki));
      sc -= due;
    }
    peek2 += lks;
    any |= pki;
    const uint32_t es2 = scs - lks;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int v = Pr::snd(p, h);
      if (v < 0) continue;
      // (index + 1) << 16 | entry of this half: one v_perm_b32
      pk[v] = __builtin_amdgcn_perm(pki, pke, h ? 0x07060302u : 0x05040100u);
      es[v] = h ? es2 >> 16 : es2 & 0xffffu;
    }
    sched_fence();
  }
  s.peek += (peek2 & 0xffffu) + (peek2 >> 16);
  // nothing due anywhere in the wave (15 % of C3's wave-ticks, mostly drain tails): the tick
  // ends here -- phase A already counted its peeks, and B, the completion check and C/D
  // would change nothing
  if (!__ballot(any != 0)) return true;
  // ---- B: receive, in-links in ascending sender rank ----------------------------------------
  // Straight-line and predicated: every register update happens on every lane (selects), only
  // the two snapshot-record stores sit in (divergent) branches -- register writes inside a
  // divergent branch make the compiler copy whole register tuples at the join.
  uint32_t tq[N];  // receiver v's first-marker triggers this tick: byte j = 0x80 | sid
  bool mkev = false;
  uint32_t* const snod = kpar()->snap_nod;
#pragma unroll
  for (int v = 0; v < N; ++v) {
    tq[v] = 0;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      if (j >= T::id(v)) continue;
      const int sj = T::src(v, j);
      const uint32_t pkj = pk[sj];
      const bool m = (pkj >> 16) == (uint32_t)(T::oix(v, j) + 1);
      // (a constant of (v, j) once the loops are unrolled, like T::id(v): a plain if)
      const bool tl = TokIn<T, P>::on(v, j);
      const bool mk = tl ? m && (pkj & 0x8000u) : m;  // (no token on this in-link: a match is a marker)
      if (tl) {
        const bool tk = m && !(pkj & 0x8000u);
        // HandleToken (node.go:174-185): tokens += data, the channel's recording cursor advances
        s.tok[v] += tk ? (int32_t)((pkj >> 8) & 0x7fu) : 0;
        s.cr[v][j >> 1] += tk ? (1u << ((j & 1) * 16)) : 0u;
      }
      // HandleMarker (node.go:149-171): the first marker of a snapshot creates the local
      // snapshot (pending = indeg - 1, nibble indeg) and triggers the broadcast; a later one
      // closes the channel (pending - 1)
      mkev = mkev || mk;
      const uint32_t sid = (pkj >> 8) & 31u;
      const uint32_t sh = (sid & 7u) * 4u;
      uint32_t pw = pd_get(s, v, sid);
      const bool nz = ((pw >> sh) & 15u) != 0;
      const bool first = mk && !nz, later = mk && nz;
      pw += first ? ((uint32_t)T::id(v) << sh) : later ? (0u - (1u << sh)) : 0u;
      pd_set(s, v, sid, pw);
      if (T::od(v) > 0) {
        tq[v] |= first ? (0x80u | sid) << (8 * j) : 0u;
        // the reference scans this sender's links after the pushes when the trigger came
        // from a lower rank: each link that was empty when it scanned it is peeked again
        if (T::src(v, j) < v) {
          s.peek += first ? es[v] : 0u;
          es[v] = first ? 0u : es[v];
        }
      }
      const uint32_t rb = plane_off(x, sid) + x.lrec;
      if (first) create_record<T, P>(x, snod, s, v, j, rb);
      // the channel's end cursor.  No store where no token travels: the 0 it would write is in the
      // record since this launch created it (TokIn)
      if (tl) {
#ifndef CLSNAP_ABL_NOSTORE
        if (later)
#else
        if (later && rb == 0xffffffffu)
#endif
          st_at(reinterpret_cast<uint16_t*>(snod), rb + node_off<T>(x, (uint32_t)v) + (uint32_t)(4 * (1 + j) + 2),
                (uint16_t)cur_get(s, v, j));
      }
    }
    sched_fence();
  }
  // ---- NotifyCompletedSnapshot (sim.go:126-131): every node's nibble is 1 ---------------
  if (__ballot(mkev)) {
#pragma unroll
    for (int w = 0; w < T::SW; ++w) {
      uint32_t all = 0x88888888u;
      if constexpr (P::SPEC) {
        // reduced over the nodes first: every node's nibble is 1 exactly when the nibble of the
        // words' OR and the nibble of their AND both are -- one zero-nibble test per word
        uint32_t por = 0u, pand = 0xffffffffu;
#pragma unroll
        for (int v = 0; v < N; ++v) {
          por |= s.pd[v][w];
          pand &= s.pd[v][w];
        }
        const uint32_t y = (por ^ 0x11111111u) | (pand ^ 0x11111111u);
        all &= ~(((y & 0x77777777u) + 0x77777777u) | y);
      } else {
#pragma unroll
        for (int v = 0; v < N; ++v) {
          const uint32_t y = s.pd[v][w] ^ 0x11111111u;  // nibble == 1 -> 0
          all &= ~(((y & 0x77777777u) + 0x77777777u) | y);
        }
      }
      uint32_t fresh = all & 0x88888888u & ~s.done[w];
      if (fresh) {
        KPar* p = kpar();
        int32_t* tick_row = p->snap_tick + x.inst * (uint32_t)p->lay.s_cap;
        while (fresh) {
          const uint32_t b = (uint32_t)__builtin_ctz(fresh);
#ifndef CLSNAP_ABL_NOTICK
          tick_row[(uint32_t)w * 8u + (b >> 2)] = s.time;
#else
          if (s.time == -7) tick_row[(uint32_t)w * 8u + (b >> 2)] = s.time;  // (timing ablation)
#endif
          s.ndone += 1;
          s.done[w] |= 1u << b;
          fresh &= fresh - 1u;
        }
      }
    }
  }
  // ---- C/D: broadcast draws in triggering-sender order, then push ------------------------
  bool trig = false;
#pragma unroll
  for (int v = 0; v < N; ++v) trig = trig || tq[v] != 0;
  if (__ballot(trig)) {
    // C: sender s's delivery went out on one of its out-links; if it triggered a broadcast at
    // that link's receiver, the broadcast draws od(receiver) delays.  Exclusive offsets in
    // sender order (sim.go:101 draws in Tick's sender order).
    uint32_t off[N];
    uint32_t acc = 0;
#pragma unroll
    for (int sv = 0; sv < N; ++sv) {
      off[sv] = acc;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        if (k >= T::od(sv)) continue;
        const int r = T::dst(sv, k), q = T::ipos(sv, k);
        acc += ((tq[r] >> (8 * q + 7)) & 1u) * (uint32_t)T::od(r);
      }
    }
    // One pass over the receivers takes each one's first trigger of the tick (no loop per
    // receiver: no loop-carried register copies); a receiver with several first markers in the
    // tick (rare) takes the others in further passes, in trigger order, so each out-link still
    // gets its pushes in order.  The status: the lowest-ranked failing node's last failing push.
    uint32_t fv = 0xffu;
    int32_t fr = 0;
    // A trigger's pushes take one of two paths, chosen for the whole wave by one guard per
    // trigger (Guard): where no lane's broadcast can fail -- the row holds all its draws and
    // none of the node's rings is at its bound -- the links run the push that cannot fail, the
    // stores under the trigger's lane mask; else every lane runs push() with all of Queue.Push's
    // failure bookkeeping, as before (mixed waves are exact by construction).  The further
    // passes (FAST = false) always take push().
    auto one = [&](auto vc, auto fastc) {
      constexpr int v = decltype(vc)::value;
      constexpr bool FAST = decltype(fastc)::value != 0;
      if constexpr (T::od(v) > 0) {
        if (__ballot(tq[v] != 0)) {
          const uint32_t q = tq[v];
          const bool on = q != 0;
          const uint32_t lb = q ? (uint32_t)__builtin_ctz(q) & 24u : 0u;  // 8 * in-link
          const uint32_t sid = (q >> lb) & 31u;
          tq[v] = q & ~(0xffu << lb);
          // (the candidates made opaque first, then selected: an asm inside a select's arm
          // became a divergent branch)
          uint32_t oc[D];
#pragma unroll
          for (int j = 0; j < D; ++j) oc[j] = j < T::id(v) ? opaque(off[T::src(v, j < T::id(v) ? j : 0)]) : 0u;
          uint32_t o = oc[0];
#pragma unroll
          for (int j = 1; j < D; ++j)
            if (j < T::id(v)) o = lb == (uint32_t)(8 * j) ? oc[j] : o;
          const int32_t k0 = s.draw + (int32_t)o;
          const uint32_t dl = delays8<T>(x, k0);  // delays k0 .. k0 + 7, where they lie
          const uint32_t mpl = opaque(0x8000u | (sid << 8));  // the marker entry's high byte, once
          bool hard = true;
          if constexpr (FAST) {
            uint32_t any = 0;
#pragma unroll
            for (int k = 0; k < D; ++k)
              if (k < T::od(v)) any |= s.hw[Pr::pr(v)][k];
            const bool past = !P::COVER && k0 + T::od(v) > x.draws;
            hard = on && (past || (any & (Guard<T>::FULL << Pr::sh(v))) != 0);
          }
          if (!FAST || __builtin_expect(__ballot(hard) != 0, 0)) {
            int32_t nf = 0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
              if (k >= T::od(v)) continue;
              push<T, SPILL>(x, s.hw[Pr::pr(v)][k], Pr::sh(v), T::off(v) + k, on, mpl, k0 + k, (dl >> (4 * k)) & 15u,
                             s.time, nf);
            }
            const bool take = nf != 0 && (uint32_t)v <= fv;
            fr = take ? nf : fr;
            fv = take ? (uint32_t)v : fv;
          } else {
            uint32_t sl[D], en[D];
#pragma unroll
            for (int k = 0; k < D; ++k) {
              if (k >= T::od(v)) continue;
              sl[k] = sure_slot<T>(x, s.hw[Pr::pr(v)][k], Pr::sh(v));
              en[k] = sure_entry(mpl, (dl >> (4 * k)) & 15u, s.time);
            }
            if (on) {  // (stores only: no register is written under the lane mask)
#pragma unroll
              for (int k = 0; k < D; ++k)
                if (k < T::od(v)) lds16_at(sl[k])[(T::off(v) + k) << (T::CAPL + 6)] = (uint16_t)en[k];
            }
            const uint32_t on01 = on ? 1u << Pr::sh(v) : 0u;
#pragma unroll
            for (int k = 0; k < D; ++k)
              if (k < T::od(v)) s.hw[Pr::pr(v)][k] += on01;
          }
        }
      }
    };
    sfor<0, N>([&](auto vc) { one(vc, IC<1>{}); });
    for (;;) {
      uint32_t rest = 0;
#pragma unroll
      for (int v = 0; v < N; ++v) rest |= tq[v];
      if (__builtin_expect(!__ballot(rest != 0), 1)) break;
      sfor<0, N>([&](auto vc) { one(vc, IC<0>{}); });
    }
    s.flag = s.flag ? s.flag : fr;
    s.draw += (int32_t)acc;
  }
  resolve(s);
  return false;
}

// Host ops name their node (and link) by uniform indices.  They are straight-line: the node's
// registers are picked with selects on the uniform index, and written back the same way, so no
// branch per node slot leaves the compiler a merge of every node's registers to resolve (those
// merges cost more registers than the tick itself).  The empty asm keeps the optimizer from
// folding a select chain over an array into one dynamically indexed access, which would move
// the instance state out of registers into scratch memory.
template <int N, class V>
__device__ __forceinline__ V pick_slot(const V (&a)[N], int32_t i) {
  V r = opaque(a[0]);
#pragma unroll
  for (int v = 1; v < N; ++v) r = v == i ? opaque(a[v]) : r;
  return r;
}
// out-link k of node a: its 16-bit head word, extracted from its pair's register
template <class T>
__device__ __forceinline__ uint32_t pick_hw(const State<T>& s, int32_t a, int32_t k) {
  uint32_t r = 0;
#pragma unroll
  for (int v = 0; v < T::N; ++v)
#pragma unroll
    for (int j = 0; j < T::D; ++j)
      if (j < T::od(v)) r = (v == a && j == k) ? opaque(hw_get(s, v, j)) : r;
  return r;
}
// ... and `inc` (0 or 1) added to its count
template <class T>
__device__ __forceinline__ void bump_hw(State<T>& s, int32_t a, int32_t k, uint32_t inc) {
#pragma unroll
  for (int v = 0; v < T::N; ++v)
#pragma unroll
    for (int j = 0; j < T::D; ++j)
      if (j < T::od(v)) s.hw[Pairs<T>::pr(v)][j] += (v == a && j == k) ? inc << Pairs<T>::sh(v) : 0u;
}

// SendTokens (node.go:112-131) of one send event: balance check, link lookup, push.
template <class T, bool SPILL>
__device__ __forceinline__ void send_one(const Ctx& x, State<T>& s, const Op& op) {
  const int32_t a = op.a, b = op.b;
  const int32_t tk = pick_slot<T::N>(s.tok, a);
  const bool insufficient = s.alive && tk < op.c;
  const bool go = s.alive && !insufficient && b >= 0;
  uint32_t hw = pick_hw(s, a, b);
  const uint32_t h0 = hw;
  int32_t nf = 0;
  const uint32_t ch = (uint32_t)(b >= 0 ? b : 0) + [&] {
    uint32_t o = 0;
#pragma unroll
    for (int v = 0; v < T::N; ++v) o = v == a ? T::off(v) : o;
    return o;
  }();
  push<T, SPILL>(x, hw, 0u, ch, go, (uint32_t)op.c << 8, s.draw, delays8<T>(x, s.draw) & 15u, s.time, nf);
  const uint32_t inc = hw - h0;  // 1 where the push landed
#pragma unroll
  for (int v = 0; v < T::N; ++v) s.tok[v] -= (v == a && go) ? op.c : 0;
  bump_hw(s, a, b, inc);
  s.flag = nf;
  if (s.alive) {
    if (insufficient) {
      s.status = ST_FATAL_INSUFFICIENT;
      s.alive = false;
    } else if (b < 0) {
      s.status = ST_FATAL_UNKNOWN_DEST;
      s.alive = false;
    } else {
      s.draw += 1;
    }
  }
  resolve(s);
}

// sim.StartSnapshot -> node.StartSnapshot (sim.go:105-123, node.go:198-212): the initiator
// records every in-channel and broadcasts.
template <class T, bool SPILL>
__device__ __forceinline__ void start_snapshot(const Ctx& x, State<T>& s, const Op& op) {
  constexpr int RW = rec_w(T::D);
  const int32_t a = op.a;
  const uint32_t sid = (uint32_t)op.b;
  const bool on = s.alive;
  int32_t id = 0, od = 0;
  uint32_t off = 0;
#pragma unroll
  for (int v = 0; v < T::N; ++v) {
    id = v == a ? T::id(v) : id;
    od = v == a ? T::od(v) : od;
    off = v == a ? T::off(v) : off;
  }
  // the pending nibble: pending = indeg (15: an initiator without in-links never completes)
  const uint32_t nib = (id == 0 ? 15u : (uint32_t)id + 1u) << ((sid & 7u) * 4u);
#pragma unroll
  for (int v = 0; v < T::N; ++v)
#pragma unroll
    for (int w = 0; w < T::SW; ++w) s.pd[v][w] |= (on && v == a && (uint32_t)w == (sid >> 3)) ? nib : 0u;
  // CreateLocalSnapshot (node.go:58-84) with every in-channel recording: one vector store
  uint32_t r[RW];
  r[0] = (uint32_t)pick_slot<T::N>(s.tok, a);
#pragma unroll
  for (int j = 0; j < RW - 1; ++j) {
    uint32_t c = 0;
    if (j < T::D) {
#pragma unroll
      for (int v = 0; v < T::N; ++v)
        if (j < T::id(v)) c = v == a ? opaque(cur_get(s, v, j)) : c;
    }
    r[1 + j] = c;
  }
  if (on) {
    const uint32_t o = plane_off(x, sid) + x.lrec + node_off<T>(x, (uint32_t)a);
    uint32_t* snod = kpar()->snap_nod;
    if constexpr (RW == 2) {
      st_at(reinterpret_cast<uint2*>(snod), o, make_uint2(r[0], r[1]));
    } else {
#pragma unroll
      for (int q = 0; q < RW; q += 4)
        st_at(reinterpret_cast<uint4*>(snod), o + 4u * q, make_uint4(r[q], r[q + 1], r[q + 2], r[q + 3]));
    }
  }
  // SendToNeighbors (node.go:97-109): one push per out-link, draws in dest order
  // One guard for the broadcast (Guard): where no lane's can fail, its links take the push that
  // cannot fail, else push() as before.
  const uint32_t dl = delays8<T>(x, s.draw);
  int32_t nf = 0;
  uint32_t any = 0;
#pragma unroll
  for (int k = 0; k < T::D; ++k)
    if (k < od) any |= pick_hw(s, a, k);
  const bool hard = on && (s.draw + od > x.draws || (any & Guard<T>::FULL) != 0);  // (extracted halves)
  if (__builtin_expect(__ballot(hard) != 0, 0)) {
#pragma unroll
    for (int k = 0; k < T::D; ++k) {
      if (k >= od) continue;  // (uniform)
      uint32_t hw = pick_hw(s, a, k);
      const uint32_t h0 = hw;
      push<T, SPILL>(x, hw, 0u, off + (uint32_t)k, on, 0x8000u | (sid << 8), s.draw + k, (dl >> (4 * k)) & 15u,
                     s.time, nf);
      bump_hw(s, a, k, hw - h0);
    }
  } else {
    const uint32_t on01 = on ? 1u : 0u;
#pragma unroll
    for (int k = 0; k < T::D; ++k) {
      if (k >= od) continue;  // (uniform)
      const uint32_t sl = sure_slot<T>(x, pick_hw(s, a, k), 0u) + ((off + (uint32_t)k) << (T::CAPL + 7));
      const uint32_t en = sure_entry(0x8000u | (sid << 8), (dl >> (4 * k)) & 15u, s.time);
      if (on) *lds16_at(sl) = (uint16_t)en;
      bump_hw(s, a, k, on01);
    }
  }
  s.flag = nf;
  if (s.alive) s.draw += op.c;
  resolve(s);
}

// ---- the event program compiled in ------------------------------------------------------------
// A replay re-runs the program its plan was built from, so cl_jit.cpp can also generate a program
// type P beside T: the op list as constants.  The tick ops cut the program into segments; P gives
// per segment the host ops (sends and snapshot starts, OP_SENDS groups as their sends in order)
// that precede its tick op, and the tick op's fields (all constexpr):
//   SPEC              true (NoProg: false, the generic kernels that read `ops`)
//   COVER             the launch's delay rows hold every draw the program can make (Guard)
//   NSEG, NARM        tick segments; arms of host ops: NSEG, + 1 for host ops after the last tick
//   h0(g)             first host op of arm g (h0(NARM): their number)
//   hk(h), ha(h), hb(h), hc(h)   host op h: OP_SEND or OP_SNAP and its fields a, b, c
//   td(g), ta(g), tb(g)          segment g's tick op: 1 for OP_DRAIN, and its fields a, b
//   ns(g)             snapshots started before segment g's tick op
// send_c / snap_c are send_one / start_snapshot with the node, link, token count and snapshot id
// as constants: they touch the node's own registers, with no select ladder over node slots and no
// op fetched, and compute the same values in the same order (the failure paths included).
template <class T, bool SPILL, int A, int B, int C>
__device__ __forceinline__ void send_c(const Ctx& x, State<T>& s) {
  const bool insufficient = s.alive && s.tok[A] < C;
  const bool go = s.alive && !insufficient && B >= 0;
  int32_t nf = 0;
  if constexpr (B >= 0) {  // (an unknown destination pushes nothing: go is false)
    push<T, SPILL>(x, s.hw[Pairs<T>::pr(A)][B], Pairs<T>::sh(A), T::off(A) + (uint32_t)B, go, (uint32_t)C << 8, s.draw,
                   delays8<T>(x, s.draw) & 15u, s.time, nf);
    // (cut here for the optimizer: over a hundred sends in a row on one high-half channel are a
    // chain of shifts, adds and selects on one register that took its value tracking tens of
    // gigabytes to see through)
    s.hw[Pairs<T>::pr(A)][B] = opaque(s.hw[Pairs<T>::pr(A)][B]);
    s.tok[A] -= go ? C : 0;
  }
  s.flag = nf;
  if (s.alive) {
    if (insufficient) {
      s.status = ST_FATAL_INSUFFICIENT;
      s.alive = false;
    } else if (B < 0) {
      s.status = ST_FATAL_UNKNOWN_DEST;
      s.alive = false;
    } else {
      s.draw += 1;
    }
  }
  resolve(s);
}

template <class T, bool SPILL, class P, int A, int SID, int C>
__device__ __forceinline__ void snap_c(const Ctx& x, State<T>& s) {
  constexpr int id = T::id(A), od = T::od(A);
  const bool on = s.alive;
  constexpr uint32_t nib = (id == 0 ? 15u : (uint32_t)id + 1u) << ((SID & 7) * 4);
  s.pd[A][SID >> 3] |= on ? nib : 0u;
  // CreateLocalSnapshot (node.go:58-84) with every in-channel recording
  if (on) create_record<T, P>(x, kpar()->snap_nod, s, A, -1, plane_off(x, (uint32_t)SID) + x.lrec);
  // SendToNeighbors (node.go:97-109): one guard, then the push that cannot fail, else push()
  int32_t nf = 0;
  if constexpr (od > 0) {
    const uint32_t dl = delays8<T>(x, s.draw);
    constexpr uint32_t mpl = 0x8000u | ((uint32_t)SID << 8);
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < od; ++k) any |= s.hw[Pairs<T>::pr(A)][k];
    const bool past = !P::COVER && s.draw + od > x.draws;
    const bool hard = on && (past || (any & (Guard<T>::FULL << Pairs<T>::sh(A))) != 0);
    if (__builtin_expect(__ballot(hard) != 0, 0)) {
#pragma unroll
      for (int k = 0; k < od; ++k)
        push<T, SPILL>(x, s.hw[Pairs<T>::pr(A)][k], Pairs<T>::sh(A), T::off(A) + (uint32_t)k, on, mpl, s.draw + k,
                       (dl >> (4 * k)) & 15u, s.time, nf);
    } else {
      uint32_t sl[od], en[od];
#pragma unroll
      for (int k = 0; k < od; ++k) {
        sl[k] = sure_slot<T>(x, s.hw[Pairs<T>::pr(A)][k], Pairs<T>::sh(A));
        en[k] = sure_entry(mpl, (dl >> (4 * k)) & 15u, s.time);
      }
      if (on) {  // (stores only: no register is written under the lane mask)
#pragma unroll
        for (int k = 0; k < od; ++k) lds16_at(sl[k])[(T::off(A) + k) << (T::CAPL + 6)] = (uint16_t)en[k];
      }
      const uint32_t on01 = on ? 1u << Pairs<T>::sh(A) : 0u;
#pragma unroll
      for (int k = 0; k < od; ++k) s.hw[Pairs<T>::pr(A)][k] += on01;
    }
  }
  s.flag = nf;
  if (s.alive) s.draw += C;
  resolve(s);
}

// The tick loop of one tick op.  TICK: `a` ticks.  DRAIN: tick until every started snapshot
// completed (at most `a` ticks, else HANG), then `b` more (test_common.go:123-137).  Per lane: a
// lane ticks while iter < until (cl_kernels.hip exec_wave).
template <class T, bool SPILL, class P>
__device__ __forceinline__ void tick_loop(const Ctx& x, State<T>& s, bool drain, int32_t a, int32_t b,
                                          int32_t n_started) {
  constexpr int N = T::N, D = T::D;
  constexpr int32_t kNoUntil = 0x7fffffff;
  int32_t until = drain ? kNoUntil : a;
  bool anyw = drain;
  for (int32_t iter = 0;; ++iter) {
    if (anyw) {
      const bool w = until == kNoUntil;
      if (w && (!s.alive || (int32_t)s.ndone >= n_started)) {
        until = iter + b;
      } else if (w && iter >= a) {
        s.status = ST_HANG;
        s.alive = false;
        until = iter;
      }
      anyw = __ballot(until == kNoUntil) != 0;
    }
    const bool act = s.alive && iter < until;
    if (!__ballot(act)) break;
    const bool idle = tick<T, SPILL, P>(x, s, act);
    if (idle && !anyw) {
      // no lane picked anything: if nothing is queued anywhere in the wave either, every
      // remaining tick of this op is empty for every lane (no peek, draw or delivery; the
      // drain tail after the last delivery, all of C3's idle wave-ticks) -- add them at once
      uint32_t q = 0;
#pragma unroll
      for (int p = 0; p < Pairs<T>::NP; ++p)
#pragma unroll
        for (int k = 0; k < D; ++k)
          if (k < Pairs<T>::nk(p)) q |= s.hw[p][k] & 0x007f007fu;
      if (!__ballot(q != 0)) {
        if (s.alive) s.time += max(0, until - (iter + 1));
        break;
      }
    }
  }
}

// The whole event program for one wave of 64 instances (slots slot_base + wave * 64 + lane).
// P = NoProg: the program is read from `ops`.  A program type P (replays of a planned program):
// the program is P's, `ops` is not read; the kernel starts from the initial state and saves no
// state image (the host launches it only so), so the resume prologue and the state-image epilogue
// are compiled out.
template <class T, bool SPILL, class P = NoProg>
__device__ __forceinline__ void program(const ExecParams& p, const Op* __restrict__ ops,
                                        const uint8_t* __restrict__ sched) {
  constexpr int N = T::N, D = T::D, RW = rec_w(T::D);
  const int32_t lane = threadIdx.x;
  const uint32_t slot = p.slot_base + blockIdx.x * (uint32_t)kWave + (uint32_t)lane;
  const bool valid = slot < (uint32_t)p.n_inst;
  const uint32_t inst = valid ? (p.inst_map ? (uint32_t)p.inst_map[slot] : slot) : 0u;
  const Layout& lay = p.lay;
  const uint32_t st = (uint32_t)p.stride;
  constexpr uint32_t capl = T::CAPL;
  const uint32_t nd = (uint32_t)(p.sched_row / 8);  // delay words (8 nibbles each)
  // 16-bit FIFO elements: lanes 0-31 in the low halves of dwords 0-31, lanes 32-63 in the high
  // halves, so each 32-lane half of a wave access hits 32 distinct banks (lane * 2 put two lanes
  // on every bank: 31M LDS bank-conflict cycles per C3 launch; 1.725 -> 1.712 ms)
  const Ctx x{(uint32_t)lane * 4u,
              ((uint32_t)lane & 31u) * 4u + ((uint32_t)lane >> 5) * 2u,
              inst,
              st,
              T::BLK ? 4u * (uint32_t)RW * ((slot >> 6) * 64u * (uint32_t)N + (slot & 63u))
                     : 4u * inst * (uint32_t)N * (uint32_t)RW,
              (4u * st * (uint32_t)N * (uint32_t)RW) >> 8,
              // (the two uniform bounds held in VGPRs: as SGPRs they were spilled to VGPR lanes and
              // read back with v_readlane at every trigger -- tick v_readlane 64 -> 28, C3 1.452 ->
              // 1.440 ms per step, gpurun_out/r06ab21)
              opaque((int32_t)(p.draws < 0x7fffffffLL ? p.draws : 0x7fffffffLL)),
              opaque(Lds<T>::DB + nd - 1)};

  Timeline tl;
  tl.begin();
  // The instance's delay row, packed to nibbles (delays are < maxDelay = 5), in the column.
  // Its 16-byte chunks are loaded kRowGroup at a time, every load of a group issued before
  // the first is used: one memory round trip per group instead of one per chunk (through the
  // slot map a wave's 64 rows are 64 scattered lines).  A group's chunks past the row's end
  // repeat its last chunk -- the same bytes packed into the same column words again.
  // A replay through the slot map has the rows packed already and block-major by slot
  // (ExecParams::sched_pk, cl_rowpack.hip): word w of the wave's rows is one contiguous access
  // that does not wait for the slot map's load, copied to the column as it is -- 16 words in
  // flight at a time.  (Lanes past the batch load nothing: the plane ends with the batch's
  // last block, and a split's second half starts mid-block.)
  if (valid && p.sched_pk) {
    constexpr uint32_t kWordGroup = 16;
    const uint32_t* pk = p.sched_pk + ((size_t)(slot >> 6) * nd * 64u + (slot & 63u));
    for (uint32_t g = 0; g < nd; g += kWordGroup) {
      uint32_t b[kWordGroup];
#pragma unroll
      for (uint32_t j = 0; j < kWordGroup; ++j) b[j] = pk[(size_t)min(g + j, nd - 1) * 64u];
#pragma unroll
      for (uint32_t j = 0; j < kWordGroup; ++j) col_wr(x, Lds<T>::DB + min(g + j, nd - 1), b[j]);
    }
  } else if (valid) {
    const uint4* row = reinterpret_cast<const uint4*>(sched + (size_t)inst * p.sched_row);
    constexpr uint32_t kRowGroup = 8;
    const uint32_t nq = nd / 2;  // (>= 1: the host pads a row to a multiple of 16 bytes)
    auto nib = [](uint32_t w) {
      return (w & 0xfu) | ((w >> 4) & 0xf0u) | ((w >> 8) & 0xf00u) | ((w >> 12) & 0xf000u);
    };
    for (uint32_t g = 0; g < nq; g += kRowGroup) {
      uint4 b[kRowGroup];
#pragma unroll
      for (uint32_t j = 0; j < kRowGroup; ++j) b[j] = row[min(g + j, nq - 1)];
#pragma unroll
      for (uint32_t j = 0; j < kRowGroup; ++j) {
        const uint32_t q = min(g + j, nq - 1);
        col_wr(x, Lds<T>::DB + 2 * q, nib(b[j].x) | (nib(b[j].y) << 16));
        col_wr(x, Lds<T>::DB + 2 * q + 1, nib(b[j].z) | (nib(b[j].w) << 16));
      }
    }
  }
  tl.mark(TL_ROW);

  State<T> s;
  s.flag = 0;
#pragma unroll
  for (int w = 0; w < T::SW; ++w) s.done[w] = 0;
#pragma unroll
  for (int v = 0; v < N; ++v) {
    s.tok[v] = p.lt.init_tok[v];
#pragma unroll
    for (int k = 0; k < (D + 1) / 2; ++k) s.cr[v][k] = 0;
#pragma unroll
    for (int w = 0; w < T::SW; ++w) s.pd[v][w] = 0;
  }
#pragma unroll
  for (int q = 0; q < Pairs<T>::NP; ++q)
#pragma unroll
    for (int k = 0; k < D; ++k) s.hw[q][k] = 0;
  s.time = s.draw = s.status = 0;
  s.peek = s.push = s.ndone = 0;
  if (P::SPEC || p.fresh) {
    // (completion ticks are stored later by this same lane: program order keeps them after)
    if (valid)
      for (int32_t sid = 0; sid < lay.s_cap; ++sid) p.snap_tick[inst * (uint32_t)lay.s_cap + sid] = -1;
  } else if (valid) {
    // resume from the node-parallel state image (cl_engine.h Layout): per node its private
    // column words and G_* registers, then the instance's completion counters
    const uint32_t* S = p.state + inst;
    const uint32_t cap = 1u << capl;
#pragma unroll
    for (int v = 0; v < N; ++v) {
      const uint32_t b = (uint32_t)v * (uint32_t)(lay.priv + G_NUM);
      for (uint32_t q = 0; q < ((uint32_t)T::od(v) << capl); ++q)
        fifo_wr(x, (T::off(v) << capl) + q, e32_to_16(S[(b + lay.w_fifo + q) * st]));
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const uint32_t lw = S[(b + lay.w_lnk + k) * st];
        if (k < T::od(v)) s.hw[Pairs<T>::pr(v)][k] |= (((lw >> 8) & 0x7fu) | ((lw & 0xffu) << 7)) << Pairs<T>::sh(v);
        if (k < T::id(v)) s.cr[v][k >> 1] |= (lw >> 16) << ((k & 1) * 16);
      }
      const uint32_t* R = S + (b + lay.priv) * st;
      s.tok[v] = (int32_t)R[G_TOKENS * st];
      const uint32_t started = R[G_STARTED * st];
      uint32_t pw[T::SW];
#pragma unroll
      for (int w = 0; w < T::SW; ++w) pw[w] = 0;
      for (int32_t sid = 0; sid < lay.s_cap; ++sid) {
        if (!((started >> sid) & 1u)) continue;
        const uint32_t pend = (S[(b + lay.w_pend + (sid >> 2)) * st] >> ((sid & 3) * 8)) & 0xffu;
        const uint32_t nib = (pend == 0 && T::id(v) == 0) ? 15u : pend + 1u;
#pragma unroll
        for (int w = 0; w < T::SW; ++w) pw[w] |= (w == (sid >> 3)) ? nib << ((sid & 7) * 4) : 0u;
      }
#pragma unroll
      for (int w = 0; w < T::SW; ++w) s.pd[v][w] = pw[w];
      if (v == 0) {
        s.time = (int32_t)R[G_TIME * st];
        s.draw = (int32_t)R[G_DRAW * st];
        s.status = (int32_t)R[G_STATUS * st];
      }
      s.peek += R[G_PEEK * st];
      s.push += R[G_PUSH * st];
    }
    const uint32_t* Dn = S + (uint32_t)N * (lay.priv + G_NUM) * st;
    for (int32_t sid = 0; sid < lay.s_cap; ++sid) {
      const uint32_t f = (int32_t)Dn[sid * st] >= N ? 8u << ((sid & 7) * 4) : 0u;
#pragma unroll
      for (int w = 0; w < T::SW; ++w) s.done[w] |= (w == (sid >> 3)) ? f : 0u;
    }
    s.ndone = Dn[lay.s_cap * st];
  }
  s.alive = valid && s.status == ST_OK;
  int32_t n_started = p.n_started_before;
  tl.mark(TL_PRO);

  if constexpr (P::SPEC) {
    // A run-time loop over the segments: each segment's host ops are straight-line code on
    // constant slots behind a uniform branch on the segment index, and the tick loop's body
    // exists once (the waves of a CU sit in different segments and share its instruction cache).
#pragma nounroll
    for (int32_t seg = 0; seg < P::NARM; ++seg) {
      bool drain = false;
      int32_t ta = 0, tb = 0;
      sfor<0, P::NARM>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        if (seg == g) {
          sfor<P::h0(g), P::h0(g + 1)>([&](auto hc) {
            constexpr int h = decltype(hc)::value;
            if constexpr (P::hk(h) == OP_SEND) send_c<T, SPILL, P::ha(h), P::hb(h), P::hc(h)>(x, s);
            else snap_c<T, SPILL, P, P::ha(h), P::hb(h), P::hc(h)>(x, s);
          });
          if constexpr (g < P::NSEG) {
            drain = P::td(g) != 0;
            ta = P::ta(g);
            tb = P::tb(g);
            n_started = P::ns(g);
          }
        }
      });
      if (P::NARM > P::NSEG && seg == P::NSEG) break;  // (host ops after the last tick op)
      tl.mark(TL_OPS);
      tick_loop<T, SPILL, P>(x, s, drain, ta, tb, n_started);
      tl.mark(TL_LOOP);
      tl.drain();
      tl.mark(TL_WAIT);
      tl.count(TL_LOOPS);
    }
  }
  // the program through the constant address space: scalar loads, so every op field is a
  // uniform SGPR value (a vector load would make the node dispatch divergent)
  typedef const __attribute__((address_space(4))) Op COp;
  COp* cops = (COp*)ops;
  for (int32_t i = p.op_begin; !P::SPEC && i < p.op_end; ++i) {
    const Op op = cops[i];
    // The tick ops first, leaving through `continue`: as the last arm of the chain below, the
    // tick loop's exit joined the other arms' paths into the next op, and the compiler kept the
    // state's registers of those paths alive across the loop -- 14 VGPRs stored to scratch
    // before every tick loop and loaded again (unused on this path) after it, behind the loop's
    // record stores.  This way the spill-free kernel has no scratch (C3: 168 -> 154 VGPRs).
    if (op.kind == OP_TICK || op.kind == OP_DRAIN) {
      tl.mark(TL_OPS);
      tick_loop<T, SPILL, P>(x, s, op.kind == OP_DRAIN, op.a, op.b, n_started);
      tl.mark(TL_LOOP);
      tl.drain();
      tl.mark(TL_WAIT);
      tl.count(TL_LOOPS);
      continue;
    }
    if (op.kind == OP_SEND) {
      send_one<T, SPILL>(x, s, op);
    } else if (op.kind == OP_SENDS) {
      // a group of sends from distinct senders: one by one is the same program (cl_engine.h)
      for (int32_t q = 1; q <= op.a; ++q) send_one<T, SPILL>(x, s, (Op)cops[i + q]);
      i += op.a;
    } else if (op.kind == OP_SNAP) {
      start_snapshot<T, SPILL>(x, s, op);
      n_started++;
    }
  }
  tl.mark(TL_OPS);

  // ---- epilogue: tokens still queued, pop counts, results, state image --------------------
  if (!valid) return;  // (never a wave's lane 0, which reports the wave's timeline)
  const uint32_t cap = 1u << capl;
  int32_t inflight = 0;
  uint32_t ptok = 0, pmk = 0, queued = 0;
#pragma unroll
  for (int v = 0; v < N; ++v) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      if (k < T::id(v) && TokIn<T, P>::on(v, k)) ptok += cur_get(s, v, k);  // (the others' cursors are 0)
      if (k >= T::od(v)) continue;
      const uint32_t w = hw_get(s, v, k), cnt = w & 0x7fu, head = w >> 7;
      const uint32_t c = T::off(v) + k;
      queued += cnt;
      for (uint32_t q = 0; q < cnt && q < cap; ++q) {
        const uint32_t e = fifo_rd(x, (c << capl) + ((head + q) & (cap - 1)));
        if (!(e & 0x8000u)) inflight += (int32_t)((e >> 8) & 0x7fu);
      }
      if (cnt > cap) {
        const uint32_t om = (1u << lay.ocap_log2) - 1;
        const uint32_t h = p.ovh[c * st + inst];
        for (uint32_t q = 0; q < cnt - cap; ++q) {
          const uint32_t e = p.ovf[((c << lay.ocap_log2) + ((h + q) & om)) * st + inst];
          if (!(e & kMarkerBit)) inflight += (int32_t)(e & 0xffffu);
        }
      }
    }
    // Queue.Pop counts (sim.go:85) derived: marker pops are indeg - pending per started snapshot
#pragma unroll
    for (int w = 0; w < T::SW; ++w)
      for (uint32_t m = s.pd[v][w]; m; m &= ~(15u << (__builtin_ctz(m) & ~3u))) {
        const uint32_t nib = (m >> (__builtin_ctz(m) & ~3u)) & 15u;
        pmk += (uint32_t)T::id(v) - (nib == 15u ? 0u : nib - 1u);
      }
  }
  int32_t* r = p.regs + (size_t)inst * R_NUM;
  r[R_TIME] = s.time;
  r[R_DRAW] = s.draw;
  r[R_STATUS] = s.status;
  r[R_NDONE] = (int32_t)s.ndone;
  r[R_PEEK] = (int32_t)s.peek;
  r[R_POP_TOK] = (int32_t)ptok;
  r[R_POP_MK] = (int32_t)pmk;
  // Queue.Push count (queue.go:18-20) derived like the pops: every packet pushed since the
  // program's start was either popped or is still queued (LDS ring or HBM spill ring)
  const uint32_t pushes = ptok + pmk + queued;
  r[R_PUSH] = (int32_t)pushes;
  r[R_INFLIGHT_TOK] = inflight;
#pragma unroll
  for (int v = 0; v < N; ++v) p.fin_tok[inst * (uint32_t)N + v] = s.tok[v];
  // (the timeline build's epilogue is the results' stores, drained; not the state image, which
  // replays do not save)
  tl.drain();
  tl.mark(TL_EPI);
  tl.flush(SPILL ? 1 : 0);
  if (P::SPEC || !p.save_state) return;
  // the node-parallel state image (peek and push counts as node 0's, the others 0)
  uint32_t* S = p.state + inst;
#pragma unroll
  for (int v = 0; v < N; ++v) {
    const uint32_t b = (uint32_t)v * (uint32_t)(lay.priv + G_NUM);
    for (int32_t k = 0; k < lay.priv; ++k) S[(b + k) * st] = 0u;
    for (uint32_t q = 0; q < ((uint32_t)T::od(v) << capl); ++q)
      S[(b + lay.w_fifo + q) * st] = e16_to_32(fifo_rd(x, (T::off(v) << capl) + q), s.time);
#pragma unroll
    for (int k = 0; k < D; ++k) {
      uint32_t lw = k < T::id(v) ? cur_get(s, v, k) << 16 : 0u;
      if (k < T::od(v)) {
        const uint32_t w = hw_get(s, v, k);
        lw |= ((w >> 7) & (cap - 1)) | ((w & 0x7fu) << 8);
      }
      S[(b + lay.w_lnk + k) * st] = lw;
    }
    uint32_t started = 0;
    for (int32_t sid = 0; sid < lay.s_cap; ++sid) {
      uint32_t pw = 0;
#pragma unroll
      for (int w = 0; w < T::SW; ++w) pw = (w == (sid >> 3)) ? s.pd[v][w] : pw;
      const uint32_t nib = (pw >> ((sid & 7) * 4)) & 15u;
      if (!nib) continue;
      started |= 1u << sid;
      const uint32_t pend = nib == 15u ? 0u : nib - 1u;
      S[(b + lay.w_pend + (sid >> 2)) * st] |= pend << ((sid & 3) * 8);
    }
    uint32_t* R = S + (b + lay.priv) * st;
    R[G_TOKENS * st] = (uint32_t)s.tok[v];
    R[G_STARTED * st] = started;
    R[G_TIME * st] = (uint32_t)s.time;
    R[G_DRAW * st] = (uint32_t)s.draw;
    R[G_STATUS * st] = (uint32_t)s.status;
    R[G_PEEK * st] = v == 0 ? s.peek : 0u;
    R[G_POP_TOK * st] = v == 0 ? ptok : 0u;  // (informational: a continuation derives them again)
    R[G_POP_MK * st] = v == 0 ? pmk : 0u;
    R[G_PUSH * st] = v == 0 ? pushes : 0u;
  }
  uint32_t* Dn = S + (uint32_t)N * (lay.priv + G_NUM) * st;
  for (int32_t sid = 0; sid < lay.s_cap; ++sid) {
    uint32_t c = 0;
#pragma unroll
    for (int v = 0; v < N; ++v) {
      uint32_t pw = 0;
#pragma unroll
      for (int w = 0; w < T::SW; ++w) pw = (w == (sid >> 3)) ? s.pd[v][w] : pw;
      c += ((pw >> ((sid & 7) * 4)) & 15u) == 1u ? 1u : 0u;
    }
    Dn[sid * st] = c;
  }
  Dn[lay.s_cap * st] = s.ndone;
}

}  // namespace lanes
}  // namespace clsnap
