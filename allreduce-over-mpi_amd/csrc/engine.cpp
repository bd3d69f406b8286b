// FlexTree AllReduce engine: runs a rank's plan on two HIP streams.
//
// Reference execution (mpi_mod.hpp:1550-1644, :1689-1715): per stage post all
// Isend/Irecv, MPI_Waitall the receives, reduce on 14 OpenMP threads,
// MPI_Waitall the sends, MPI_Barrier — no overlap between communication and
// reduction, a global barrier every stage, host buffers.
//
// Here (device-resident, nothing blocks the host):
//   comm stream : the stage's transfers, cut into pieces of `chunk` elements
//                 (piece c of every block of the stage = one p2p group);
//   reduce stream: the reduce kernel for piece c starts as soon as piece c of
//                 the stage's receives has landed (event), while piece c+1 is
//                 still on the wire;
//   cross-stage : piece c of stage s+1's transfers waits only for piece c of
//                 the latest reducing stage (what it sends, or the scratch it
//                 overwrites two stages later, depends on nothing else);
//   scratch     : compact, two halves alternating per stage, grow-only, HBM.
// The caller's stream is joined at entry and at exit with events, so the call
// is stream-ordered like any other HIP operation.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <cstdio>

#include "engine_state.h"

using ftar::hip_ignore;

namespace ftar {

// phase timing: one timing event per boundary, on the stream that reaches it
ftar_status_t mark(ftar_comm* c, const std::string& name, hipStream_t s) {
  if (!c->phase_timing) return FTAR_SUCCESS;
  if (c->nmarks == c->tev.size()) {
    hipEvent_t e;
    FTAR_CHECK_HIP(hipEventCreate(&e));
    c->tev.push_back(e);
    c->tnames.emplace_back();
  }
  c->tnames[c->nmarks] = name;
  FTAR_CHECK_HIP(hipEventRecord(c->tev[c->nmarks++], s));
  return FTAR_SUCCESS;
}

ftar_status_t grow_events(ftar_comm* c, size_t n) {
  if (c->capturing) {  // a fresh set for this captured call; the uncaptured set stays as it is
    for (hipEvent_t e : c->events) c->captured_events.push_back(e);
    c->events.clear();
  }
  while (c->events.size() < n) {
    hipEvent_t e;
    FTAR_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->events.push_back(e);
  }
  return FTAR_SUCCESS;
}

ftar_status_t fork_streams(hipStream_t stream, hipEvent_t ev, std::initializer_list<hipStream_t> streams) {
  FTAR_CHECK_HIP(hipEventRecord(ev, stream));
  for (hipStream_t s : streams) FTAR_CHECK_HIP(hipStreamWaitEvent(s, ev, 0));
  return FTAR_SUCCESS;
}

ftar_status_t join_streams(hipStream_t stream, std::initializer_list<Join> joins) {
  for (const Join& j : joins)
    if (j.record) FTAR_CHECK_HIP(hipEventRecord(j.ev, j.s));
  for (const Join& j : joins) FTAR_CHECK_HIP(hipStreamWaitEvent(stream, j.ev, 0));
  return FTAR_SUCCESS;
}

// The reduce stream on `cus` of the device's CUs (0 or >= all: every CU), so
// the transport's own kernels on the comm stream (RCCL's p2p kernels, the
// local transport's copies) always find free CUs while a piece's fold runs:
// the one-shot reduce grids otherwise fill every CU.  The CUs kept are spread
// evenly over the mask (CU i is kept iff floor((i+1)*cus/N) > floor(i*cus/N)),
// so every XCD keeps its share whichever way the mask bits map to XCDs.
// hipExtStreamCreateWithCUMask makes a blocking stream (it synchronises with
// the legacy NULL stream) on a hardware queue of its own, the price of the knob.
// Refused on RCCL communicators (Transport::masked_reduce_stream_ok): two runs
// of the RCCL stress driver stalled ranks inside the first call after the knob
// moved from 0 to a CU share (profiles/r04/stress_soak/).
ftar_status_t set_reduce_cus(ftar_comm* c, int cus) {
  int total = 0;
  FTAR_CHECK_HIP(hipDeviceGetAttribute(&total, hipDeviceAttributeMultiprocessorCount, c->device));
  if (cus <= 0 || cus >= total) cus = 0;
  if (cus && c->tp && !c->tp->masked_reduce_stream_ok()) {
    set_error("the reduce stream cannot be CU-masked on a " + std::string(c->tp->name()) +
                  " communicator (ftar_comm_set_reduce_cus / FTAR_REDUCE_CUS): a masked stream is a blocking "
                  "stream on a hardware queue of its own, and over RCCL it stalled ranks (DESIGN §5.1); "
                  "0 (every CU) is the only value accepted there",
              __FILE__, __LINE__);
    return FTAR_ERR_UNSUPPORTED;
  }
  if (cus == c->reduce_cus && c->red_s) return FTAR_SUCCESS;
  hipStream_t fresh = nullptr;
  if (cus == 0) {
    FTAR_CHECK_HIP(hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking));
  } else {
    std::vector<uint32_t> mask((size_t)(total + 31) / 32, 0u);
    for (int i = 0; i < total; ++i)
      if ((long)(i + 1) * cus / total > (long)i * cus / total) mask[(size_t)i / 32] |= 1u << (i % 32);
    FTAR_CHECK_HIP(hipExtStreamCreateWithCUMask(&fresh, (uint32_t)mask.size(), mask.data()));
  }
  if (c->red_s) {
    hip_ignore(hipStreamSynchronize(c->red_s));
    hip_ignore(hipStreamDestroy(c->red_s));
  }
  c->red_s = fresh;
  c->reduce_cus = cus;
  trace("rank %d: reduce stream on %d of %d CUs", c->rank, cus ? cus : total, total);
  return FTAR_SUCCESS;
}

// The form a reduce-scatter, an all-gather and a peer mode make (ftar_form_t), or -2 for a mix no form names.
int form_for(int reduce_scatter, int allgather, int peer) {
  if (peer == FTAR_PEER_READ) return FTAR_FORM_PEER_READ;
  if (peer == FTAR_PEER_WRITE) return FTAR_FORM_PEER_WRITE;
  if (reduce_scatter == FTAR_RS_STAGES) return allgather == FTAR_AG_STAGES ? FTAR_FORM_STAGES : -2;
  if (allgather == FTAR_AG_DIRECT) return FTAR_FORM_DIRECT;
  return allgather == FTAR_AG_COLLECTIVE ? FTAR_FORM_COLLECTIVE : -2;
}
int form_of(const ftar_comm* c) { return form_for(c->reduce_scatter, c->allgather, c->peer_direct); }

// The one decision of a call.  Host buffers on a p2p transport run staged whatever the peer mode; without p2p
// only the peer forms move anything.
CallPath call_path(bool host, bool p2p, int peer_mode, bool eligible, bool pipeline, bool several_pieces) {
  if (!host && peer_mode && eligible) return CallPath::PeerDevice;
  if (host && peer_mode == FTAR_PEER_READ && !p2p && eligible && pipeline && several_pieces)
    return CallPath::PeerHostPipelined;
  if (host && peer_mode && !p2p && eligible) return CallPath::PeerHostWhole;
  return p2p ? CallPath::Staged : CallPath::Refused;
}

// "auto" | "direct" | "stages" | "collective" | "peer-read" | "peer-write"; -3 = none of them
int form_from_name(const std::string& m) {
  if (m == "auto" || m.empty()) return FTAR_FORM_AUTO;
  if (m == "direct") return FTAR_FORM_DIRECT;
  if (m == "stages") return FTAR_FORM_STAGES;
  if (m == "collective") return FTAR_FORM_COLLECTIVE;
  if (m == "peer-read" || m == "read") return FTAR_FORM_PEER_READ;
  if (m == "peer-write" || m == "write") return FTAR_FORM_PEER_WRITE;
  return -3;
}

// The settings of one form (the engine's three knobs): all-gather, reduce-scatter, peer mode.
void form_settings(int form, int* ag, int* rs, int* peer) {
  *ag = form == FTAR_FORM_STAGES ? FTAR_AG_STAGES : form == FTAR_FORM_COLLECTIVE ? FTAR_AG_COLLECTIVE : FTAR_AG_DIRECT;
  *rs = form == FTAR_FORM_STAGES ? FTAR_RS_STAGES : FTAR_RS_DIRECT;
  *peer = form == FTAR_FORM_PEER_READ ? FTAR_PEER_READ : form == FTAR_FORM_PEER_WRITE ? FTAR_PEER_WRITE : FTAR_PEER_OFF;
}

void set_form(ftar_comm* c, int form) {
  c->form = form;
  if (form >= FTAR_FORM_DIRECT) form_settings(form, &c->allgather, &c->reduce_scatter, &c->peer_direct);
  else if (form == FTAR_FORM_AUTO) c->peer_direct = FTAR_PEER_OFF;
}

// the host-buffer path's copy streams, created at the first host-buffer call (see comm_setup_local)
// FTAR_DEBUG_HOST_COPY_PRIORITY=1 (diagnostic, tools/host_comm_stress.py): both at the highest priority,
// which the runtime puts on hardware queues of their own -- the configuration of round 5's one
// c4_host_read mismatch
ftar_status_t ensure_host_streams(ftar_comm* c) {
  static const bool prio = getenv("FTAR_DEBUG_HOST_COPY_PRIORITY") && atoi(getenv("FTAR_DEBUG_HOST_COPY_PRIORITY"));
  for (hipStream_t* s : {&c->h2d_s, &c->d2h_s}) {
    if (*s) continue;
    if (prio) {
      int least = 0, greatest = 0;
      FTAR_CHECK_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
      FTAR_CHECK_HIP(hipStreamCreateWithPriority(s, hipStreamNonBlocking, greatest));
    } else {
      FTAR_CHECK_HIP(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
    }
  }
  return FTAR_SUCCESS;
}

ftar_status_t agree_settings(ftar_comm* c, bool failed = false);

namespace {
// the local part of a communicator's bring-up: streams, events, settings from the environment
ftar_status_t comm_setup_local(ftar_comm* c) {
  FTAR_RETURN_IF(cost_file_status());  // a calibration file that does not parse fails loudly, on every rank
  FTAR_CHECK_HIP(hipSetDevice(c->device));
  FTAR_CHECK_HIP(hipStreamCreateWithFlags(&c->comm_s, hipStreamNonBlocking));
  if (const char* rc = getenv("FTAR_REDUCE_CUS")) FTAR_RETURN_IF(set_reduce_cus(c, atoi(rc)));
  else FTAR_CHECK_HIP(hipStreamCreateWithFlags(&c->red_s, hipStreamNonBlocking));
  // the H2D / D2H streams exist only once a host-buffer call needs them (ensure_host_streams): a process
  // has 4 hardware queues by default and streams beyond that share them (tools/rccl_order/queue_probe), so a
  // device-resident user keeps the comm and reduce streams on queues of their own
  FTAR_CHECK_HIP(hipEventCreateWithFlags(&c->done_ev, hipEventDisableTiming));
  FTAR_CHECK_ALLOC(hipMalloc(reinterpret_cast<void**>(&c->amax_buf), (1 + (size_t)c->nranks) * sizeof(unsigned)));
  if (const char* pd = getenv("FTAR_PEER_DIRECT")) {
    const std::string m(pd);
    c->peer_direct = m == "write" ? FTAR_PEER_WRITE : m == "read" ? FTAR_PEER_READ
                     : std::max(0, std::min(2, atoi(pd)));
  }
  if (const char* hp = getenv("FTAR_HOST_PEER_PIPELINE")) c->host_peer_pipeline = atoi(hp) != 0;
  if (const char* rr = getenv("FTAR_RCCL_REGISTER")) c->rccl_reg = atoi(rr) != 0;
  const char* hcb = getenv("FTAR_HOST_CHUNK_BYTES");
  c->host_chunk_bytes = hcb ? strtoull(hcb, nullptr, 0) : kDefaultHostChunkBytes;
  if (c->host_chunk_bytes && c->host_chunk_bytes < 256) c->host_chunk_bytes = 256;
  if (const char* rs = getenv("FTAR_REDUCE_SCATTER"))
    c->reduce_scatter = std::string(rs) == "stages" ? FTAR_RS_STAGES : FTAR_RS_DIRECT;
  if (const char* ag = getenv("FTAR_ALLGATHER")) {
    const std::string m(ag);
    c->allgather = m == "stages" ? FTAR_AG_STAGES : m == "collective" ? FTAR_AG_COLLECTIVE : FTAR_AG_DIRECT;
  }
  // any explicit data-movement setting fixes the form; FTAR_FORM names one (or "auto") outright
  if (getenv("FTAR_PEER_DIRECT") || getenv("FTAR_REDUCE_SCATTER") || getenv("FTAR_ALLGATHER")) c->form = form_of(c);
  if (const char* fm = getenv("FTAR_FORM")) {
    const int f = form_from_name(fm);
    if (f == -3) {
      set_error(std::string("FTAR_FORM=") + fm + ": expected auto, direct, stages, collective, peer-read or peer-write",
                __FILE__, __LINE__);
      return FTAR_ERR_INVALID_ARG;
    }
    set_form(c, f);
  }
  if (!c->tp->async_p2p()) c->form = form_of(c);  // a host-bootstrapped communicator keeps its peer form
  const char* cb = getenv("FTAR_CHUNK_BYTES");
  const size_t cbv = cb ? strtoull(cb, nullptr, 0) : 0;
  c->chunk_bytes = cbv ? std::max<size_t>(256, cbv & ~size_t(255)) : 0;
  return FTAR_SUCCESS;
}
}  // namespace

// A host-bootstrapped communicator compares its settings at bring-up, and a rank whose local bring-up
// failed still takes part in that host collective, flagging its failure, so no peer is left waiting in it
// (ADVICE r3); an RCCL one compares them at its first call (first_contact), so a rank whose RCCL bring-up
// failed leaves no peer waiting in a collective inside ftar_comm_init_rank.
ftar_status_t comm_setup(ftar_comm* c) {
  ftar_status_t st = comm_setup_local(c);
  if (!c->tp->async_p2p()) {
    const std::string local_err = st == FTAR_SUCCESS ? "" : last_error();
    const ftar_status_t ag = agree_settings(c, st != FTAR_SUCCESS);
    if (st != FTAR_SUCCESS) set_error(local_err, __FILE__, __LINE__);
    else st = ag;
    if (st == FTAR_SUCCESS) c->settings_agreed = true;
  }
  return st;
}

// The environment-derived settings that shape the messages every rank posts (piece sizes, data-movement
// forms) and the topology choice (FT_TOPO / FT_LONELY, the cost model and its constants) must be alike on
// every rank: a rank pieced differently from its peers posts transfers they do not match.  Compared once
// (collective: at bring-up, or an RCCL communicator's first call), so a mismatched launch fails every rank
// instead of hanging a call.
// Setters (ftar_comm_set_*, ftar_cost_set_params) must likewise be called alike, as RCCL's own
// configuration must.
ftar_status_t agree_settings(ftar_comm* c, bool failed) {
  auto h = [](const char* v) {  // FNV-1a of an environment string ("" = unset)
    uint64_t x = 1469598103934665603ull;
    for (const char* p = v ? v : ""; *p; ++p) x = (x ^ (unsigned char)*p) * 1099511628211ull;
    return x;
  };
  ftar_cost_params_t k;
  ftar_cost_get(&k);
  uint64_t cfg[10 + sizeof k / 8] = {(uint64_t)c->chunk_bytes, (uint64_t)c->host_chunk_bytes,
                                     (uint64_t)c->peer_direct, (uint64_t)c->host_peer_pipeline,
                                     (uint64_t)c->reduce_scatter, (uint64_t)c->allgather, (uint64_t)(int64_t)c->form,
                                     h(getenv("FT_TOPO")), h(getenv("FT_LONELY")), h(getenv("FTAR_COST_MODEL"))};
  static_assert(sizeof k % 8 == 0, "cost params are doubles");
  memcpy(&cfg[10], &k, sizeof k);
  if (failed) cfg[0] = ~uint64_t(0);  // this rank's bring-up failed: no peer can match it
  bool same = true;
  FTAR_RETURN_IF(c->tp->agree(cfg, sizeof cfg, &same));
  if (failed) return FTAR_ERR_INTERNAL;
  if (!same) {
    set_error("another rank's bring-up failed, or the ranks disagree on FTAR_CHUNK_BYTES / FTAR_HOST_CHUNK_BYTES / "
              "FTAR_PEER_DIRECT / FTAR_HOST_PEER_PIPELINE / FTAR_REDUCE_SCATTER / FTAR_ALLGATHER / FTAR_FORM / FT_TOPO / FT_LONELY / "
              "the cost model or its constants: launch every rank with the same environment",
              __FILE__, __LINE__);
    return FTAR_ERR_INVALID_ARG;
  }
  return FTAR_SUCCESS;
}

// A communicator's first contact: the settings agreement, then (RCCL) one byte each way with every peer so
// that RCCL's lazy p2p connection handshakes happen here and no later call's ncclGroupEnd blocks on one.
// Where the transport may block the host in it (RCCL), it runs on a helper thread that the caller waits for
// with a deadline, FTAR_FIRST_CONTACT_TIMEOUT_S (default 600 s; 0 = no helper, no deadline): a peer that
// never shows up, or a transport stuck at its first transfer, then fails the call with FTAR_ERR_TIMEOUT
// instead of hanging it (bench.py's RCCL preflight relies on it), and the communicator is
// marked broken -- every later call fails the same way and teardown aborts the transport.
ftar_status_t first_contact(ftar_comm* c) {
  if (c->broken) {
    set_error("this communicator's first contact timed out earlier: it is unusable (destroy it)", __FILE__, __LINE__);
    return FTAR_ERR_TIMEOUT;
  }
  const char* e = getenv("FTAR_FIRST_CONTACT_TIMEOUT_S");
  const double limit = e && *e ? atof(e) : 600.0;
  auto run = [](ftar_comm* cc) {
    ftar_status_t st = agree_settings(cc);
    if (st == FTAR_SUCCESS) st = cc->tp->connect_peers(cc->rank);
    return st;
  };
  if (!c->tp->first_contact_blocks() || limit <= 0) return run(c);
  auto fc = std::make_shared<FirstContact>();
  c->contact = fc;
  c->contact_thread = std::thread([c, fc, run] {
    hip_ignore(hipSetDevice(c->device));
    const ftar_status_t st = run(c);
    std::lock_guard<std::mutex> g(fc->mu);
    fc->st = st;
    fc->err = st == FTAR_SUCCESS ? "" : last_error();
    fc->done = true;
    fc->cv.notify_all();
  });
  std::unique_lock<std::mutex> lk(fc->mu);
  if (!fc->cv.wait_for(lk, std::chrono::duration<double>(limit), [&] { return fc->done; })) {
    c->broken = true;
    set_error("first contact of the RCCL communicator (settings all-gather, p2p connections) not complete after " +
                  std::to_string(limit) + " s: a peer is missing or the transport is stuck; the communicator is "
                  "unusable (FTAR_FIRST_CONTACT_TIMEOUT_S)",
              __FILE__, __LINE__);
    return FTAR_ERR_TIMEOUT;
  }
  const ftar_status_t st = fc->st;
  const std::string err = fc->err;
  lk.unlock();
  c->contact_thread.join();
  if (st != FTAR_SUCCESS) set_error("first contact: " + err, __FILE__, __LINE__);
  return st;
}

// The topology of a call with topo == NULL, from the environment AT THIS CALL
// (get_stages, mpi_mod.hpp:1419-1486, re-run by every MPI_Allreduce_FT call,
// :1732).  FT_TOPO and FT_LONELY both unset (or FT_LONELY "0"): *is_auto, the
// cost model chooses (the reference exit(1)s here for P > 1).
// Anything else must parse for this communicator's size, or the call fails
// with FTAR_ERR_INVALID_TOPO before it enqueues anything (the reference:
// "invalid FT_TOPO" and exit(1), :1471-1475) -- on every rank alike, since
// every rank reads the same environment.
static ftar_status_t env_topology(ftar_comm* c, bool* is_auto, Topology* out) {
  const char* et = getenv("FT_TOPO");
  const char* el = getenv("FT_LONELY");
  const std::string st = et ? et : "", sl = el ? el : "";
  if (!c->env_seen || st != c->env_topo || sl != c->env_lonely) {
    c->env_seen = true;
    c->env_topo = st;
    c->env_lonely = sl;
    c->env_auto = st.empty() && (sl.empty() || sl == "0");
    c->env_status = FTAR_SUCCESS;
    if (!c->env_auto) {
      ftar_topo_t t;
      c->env_status = ftar_topo_parse(st.c_str(), sl.c_str(), c->nranks, &t);
      if (c->env_status == FTAR_SUCCESS) c->env_status = to_topology(&t, c->nranks, &c->env_t);
      if (c->env_status != FTAR_SUCCESS) c->env_status = FTAR_ERR_INVALID_TOPO;
    }
  }
  if (c->env_status != FTAR_SUCCESS) {
    set_error("invalid FT_TOPO '" + st + "' / FT_LONELY '" + sl + "' for " + std::to_string(c->nranks) + " ranks",
              __FILE__, __LINE__);
    return c->env_status;
  }
  *is_auto = c->env_auto;
  if (!c->env_auto) *out = c->env_t;
  return FTAR_SUCCESS;
}

// false: the communicator must not be freed (its first contact's helper thread may still be inside the
// transport after the abort; it is left behind with the memory it uses)
bool comm_teardown(ftar_comm* c) {
  hip_ignore(hipSetDevice(c->device));
  if (c->contact_thread.joinable()) {
    if (c->broken && c->tp) c->tp->abort();  // ncclCommAbort: the stuck first contact returns with an error
    bool done = false;
    {
      std::unique_lock<std::mutex> lk(c->contact->mu);
      done = c->contact->cv.wait_for(lk, std::chrono::seconds(c->broken ? 10 : 600), [&] { return c->contact->done; });
    }
    if (!done) {
      c->contact_thread.detach();
      return false;
    }
    c->contact_thread.join();
  }
  // A broken communicator's transport is aborted and its first-contact helper has returned: everything is
  // released as usual, only its streams are not waited for (nothing on them is waited for after an abort)
  if (!c->broken)
    for (hipStream_t st : {c->comm_s, c->red_s, c->h2d_s, c->d2h_s})
      if (st) hip_ignore(hipStreamSynchronize(st));
  if (c->tp) {
    c->tp->unmap_peers(&c->xpeers, c->rank);
    for (auto& r : c->regs) {
      c->tp->unmap_peers(&r.second.peers, c->rank);
      c->tp->rccl_deregister(r.second.rccl);
    }
    if (c->scratch_rccl) c->tp->rccl_deregister(c->scratch_rccl);
    c->scratch_rccl = nullptr;
  }
  c->regs.clear();
  if (c->xbuf) {
    forget_token(c->xbuf);
    hip_ignore(hipFree(c->xbuf));
  }
  c->tp.reset();
  for (hipStream_t t : c->dma_s) hip_ignore(hipStreamDestroy(t));
  for (hipEvent_t e : c->dma_ev) hip_ignore(hipEventDestroy(e));
  if (c->dma_fork) hip_ignore(hipEventDestroy(c->dma_fork));
  if (c->done_ev) hip_ignore(hipEventDestroy(c->done_ev));
  for (auto e : c->events) hip_ignore(hipEventDestroy(e));
  for (auto e : c->captured_events) hip_ignore(hipEventDestroy(e));
  for (auto e : c->tev) hip_ignore(hipEventDestroy(e));
  if (c->scratch) hip_ignore(hipFree(c->scratch));
  if (c->amax_buf) hip_ignore(hipFree(c->amax_buf));
  if (c->staging) hip_ignore(hipFree(c->staging));
  if (c->glog.host) hip_ignore(hipHostFree(c->glog.host));
  if (c->glog.dev) hip_ignore(hipFree(c->glog.dev));
  for (hipStream_t st : {c->comm_s, c->red_s, c->h2d_s, c->d2h_s})
    if (st) hip_ignore(hipStreamDestroy(st));
  return true;
}

namespace {

// What the call runs: the topology, form and piece the caller fixed, the rest from the execution model
// (cost_model.cpp), cached per communicator.  The same inputs on every rank give the same choice: the
// model's constants are compared across ranks at the first call (agree_settings).  Peer forms are
// candidates only for device buffers (captured or not: a capture takes the choice its warm-up call took),
// only at P > 1, and only once their rates are set.
ftar_status_t decide_exec(ftar_comm* c, Topology* t, bool topo_auto, size_t bytes, bool host, ExecChoice* out) {
  int flags = 0;
  if (topo_auto) flags |= FTAR_CHOOSE_TOPO;
  if (c->form == FTAR_FORM_AUTO && c->tp->async_p2p()) {
    flags |= FTAR_CHOOSE_FORM;
    // the same choice captured or not: a warm-up call of the shape sizes exactly what its capture uses
    if (!host && c->nranks > 1) flags |= FTAR_CHOOSE_PEER;
  }
  if (!c->chunk_bytes && !host) flags |= FTAR_CHOOSE_CHUNK;
  // a fixed mix of settings no form names is priced as the form of its reduce-scatter
  const int fixed_form = c->form >= FTAR_FORM_DIRECT ? c->form
                         : c->reduce_scatter == FTAR_RS_STAGES ? FTAR_FORM_STAGES : FTAR_FORM_DIRECT;
  const size_t fixed_chunk = host ? 0 : c->chunk_bytes;
  const std::string key = std::to_string(bytes) + "/" + std::to_string(flags) + "/" + t->key() + "/" +
                          std::to_string(fixed_form) + "/" + std::to_string(fixed_chunk) + "/" +
                          std::to_string(cost_generation());
  auto it = c->exec_cache.find(key);
  if (it == c->exec_cache.end()) {
    ExecChoice ch;
    ftar_status_t st = choose_exec(c->nranks, bytes, flags, *t, fixed_form, fixed_chunk, &ch);
    if (st != FTAR_SUCCESS) {  // nothing the model can price (e.g. P > FTAR_MAX_K one-round): as configured
      ch.topo = *t;
      ch.form = fixed_form;
      ch.chunk = fixed_chunk;
      ch.seconds = -1;
      if (flags & FTAR_CHOOSE_TOPO) {  // the topology the default data movement would take (ftar_topo_choose)
        ExecChoice d;
        if (choose_exec(c->nranks, bytes, FTAR_CHOOSE_TOPO | FTAR_CHOOSE_CHUNK, *t, FTAR_FORM_DIRECT, 0, &d) ==
            FTAR_SUCCESS) {
          ch.topo = d.topo;
        } else {  // the ring runs at any size
          ch.topo = Topology();
          ch.topo.ring = true;
          ch.topo.widths = {1};
        }
      }
    }
    if (c->exec_cache.size() > 256) c->exec_cache.clear();
    it = c->exec_cache.emplace(key, ch).first;
  }
  *out = it->second;
  *t = out->topo;
  return FTAR_SUCCESS;
}

// The call's cached plan; check_world once per (topology, count, form).
ftar_status_t resolve_plan(ftar_comm* c, const Topology& t, size_t count, const Form& form, const Plan** out) {
  const std::string key = t.key() + "/" + std::to_string(count) + "/ag" + std::to_string(form.allgather) + "/rs" +
                          std::to_string(form.reduce_scatter);
  auto it = c->plans.find(key);
  if (it == c->plans.end()) {
    auto p = std::make_shared<Plan>();
    FTAR_RETURN_IF(check_world(t, c->nranks, count, form));
    FTAR_RETURN_IF(build_plan(t, c->nranks, c->rank, count, p.get(), form));
    if (c->plans.size() > 64) c->plans.clear();
    it = c->plans.emplace(key, p).first;
  }
  if (it->second->max_k > FTAR_MAX_K) return FTAR_ERR_UNSUPPORTED;
  *out = it->second.get();
  return FTAR_SUCCESS;
}

// What one call does, resolved once (resolve_call): the executor reads it, nothing is decided again.
struct Call {
  Topology topology;
  ExecChoice ex;
  Form form;
  const Plan* plan = nullptr;
  int peer_mode = FTAR_PEER_OFF;
  size_t host_piece = 0;  // elements per piece of peer_allreduce_host (host buffers, no p2p), else 0
  CallPath path = CallPath::Refused;
};

// The call's decision: call->topology holds the topology the caller or the environment fixed (topo_auto: none
// did, the execution model chooses -- or, under FTAR_COST_MODEL=reference, the reference's own model's width
// list); then the model's choice, the form, the plan and the path.  Writes what runs to c->last_exec
// (ftar_comm_last_exec), also for a call that is then refused.
ftar_status_t resolve_call(ftar_comm* c, bool topo_auto, size_t count, size_t esz, bool host, Call* call) {
  const bool p2p = c->tp->async_p2p();
  const char* m = getenv("FTAR_COST_MODEL");
  if (topo_auto && m && !strcmp(m, "reference")) {
    ftar_topo_t ch;
    FTAR_RETURN_IF(ftar_topo_choose(c->nranks, count * esz, &ch));
    FTAR_RETURN_IF(to_topology(&ch, c->nranks, &call->topology));
    topo_auto = false;
  }
  const ExecChoice& ex = call->ex;
  FTAR_RETURN_IF(decide_exec(c, &call->topology, topo_auto, count * esz, host, &call->ex));
  Form& form = call->form;
  form.allgather = c->allgather;
  form.reduce_scatter = c->reduce_scatter;
  call->peer_mode = c->peer_direct;
  if (c->form == FTAR_FORM_AUTO && p2p) form_settings(ex.form, &form.allgather, &form.reduce_scatter, &call->peer_mode);
  if (host && form.allgather == FTAR_AG_COLLECTIVE) form.allgather = FTAR_AG_DIRECT;  // D2H needs pieces
  FTAR_RETURN_IF(resolve_plan(c, call->topology, count, form, &call->plan));
  const Plan& plan = *call->plan;
  call->host_piece = host && !p2p ? host_peer_piece(c, plan.split, esz) : 0;
  call->path = call_path(host, p2p, call->peer_mode, peer_eligible(plan), c->host_peer_pipeline,
                         call->host_piece < plan.split);
  // what runs (ftar_comm_last_exec): a peer form exactly on the three peer paths -- rows 1-3 of call_path are
  // "peer mode set, plan eligible, and device buffers or no p2p", each way round -- else the form of the
  // settings' reduce-scatter and the plan's all-gather (host buffers on a p2p transport, a plan no peer kernel
  // runs, the collective all-gather a ring or host buffers replace)
  const bool peer = call->path == CallPath::PeerDevice || call->path == CallPath::PeerHostPipelined ||
                    call->path == CallPath::PeerHostWhole;
  from_topology(call->topology, &c->last_exec.topo);
  c->last_exec.form = form_for(form.reduce_scatter, plan.allgather, peer ? call->peer_mode : FTAR_PEER_OFF);
  // the piece: none on a whole-bucket peer path; the staged executor puts the host piece it runs
  c->last_exec.chunk_bytes = call->path == CallPath::PeerHostPipelined ? call->host_piece * esz : peer ? 0 : ex.chunk;
  c->last_exec.seconds = ex.seconds;
  c->last_exec.tied = ex.tied;
  c->last_exec.tie_broken_by = ex.tie_broken_by;
  if (!p2p) {
    // A host-bootstrapped communicator's paths differ in their host barriers (peer read: 3, write: 3,
    // host buffers pipelined: m + 2, whole bucket: 3), so every rank must take the same one with the same
    // pieces: the settings that choose it are compared first, and a mismatch fails the call on every rank
    //  instead of pairing barriers of different phases.
    const uint64_t cfg[6] = {(uint64_t)call->peer_mode, (uint64_t)c->allgather, (uint64_t)c->reduce_scatter,
                             (uint64_t)host, host ? (uint64_t)c->host_peer_pipeline : 0, (uint64_t)call->host_piece};
    bool same = true;
    FTAR_RETURN_IF(c->tp->agree(cfg, sizeof cfg, &same));
    if (!same) {
      set_error("ranks disagree on the peer form, all-gather/reduce-scatter form, FTAR_HOST_PEER_PIPELINE or the "
                "host piece size (FTAR_HOST_CHUNK_BYTES): set them alike on every rank",
                __FILE__, __LINE__);
      return FTAR_ERR_INVALID_ARG;
    }
  }
  return FTAR_SUCCESS;
}

}  // namespace

// Grow-only device buffer; before freeing the old one, drain the streams whose
// earlier work may still touch it.
ftar_status_t ensure_buffer(void** buf, size_t* have, size_t need, std::initializer_list<hipStream_t> users) {
  if (need <= *have) return FTAR_SUCCESS;
  if (*buf) {
    for (hipStream_t st : users)
      if (st) FTAR_CHECK_HIP(hipStreamSynchronize(st));  // (a stream not created yet has nothing in flight)
    FTAR_CHECK_HIP(hipFree(*buf));
    *buf = nullptr;
    *have = 0;
  }
  FTAR_CHECK_ALLOC(hipMalloc(buf, need));
  *have = need;
  return FTAR_SUCCESS;
}

// What one call runs, under the communicator's lock (allreduce): the early exits in the reference's order,
// one decision (resolve_call), one executor.
ftar_status_t allreduce_locked(const void* sendbuf, void* recvbuf, size_t count, ftar_dtype_t dt, ftar_op_t op,
                               const ftar_topo_t* topo, ftar_comm* c, hipStream_t stream, const HostIO* host) {
  const size_t esz = dtype_size(dt);
  if (sendbuf == recvbuf) sendbuf = nullptr;
  // The call's topology: the argument, or FT_TOPO/FT_LONELY read at this call; both unset: topo_auto.  It is
  // checked first, as get_stages runs before the P <= 1 copy (mpi_mod.hpp:1732-1746)
  Call call;
  bool topo_auto = false;
  FTAR_RETURN_IF(topo ? to_topology(topo, c->nranks, &call.topology) : env_topology(c, &topo_auto, &call.topology));
  if (c->broken) return first_contact(c);  // reports why
  if (!c->settings_agreed && !c->capturing) {  // an RCCL communicator's first call (see comm_setup); a
    FTAR_RETURN_IF(first_contact(c));          // 1-rank one too, which exercises the same all-gather
    c->settings_agreed = true;
  }
  if (c->nranks == 1 && c->amax_cur) {  // an amax call: the copy becomes a k = 1 amax fold (in place without sendbuf)
    const void* src = sendbuf ? sendbuf : recvbuf;
    const double one = 1.0;  // AVG of one rank: r = 1
    FoldCall f;
    f.srcs = &src; f.k = 1; f.dst = recvbuf; f.count = count; f.dt = dt;
    f.stream = stream; f.scale = &one; f.amax = c->amax_cur;
    return count ? launch_reduce(f) : FTAR_SUCCESS;
  }
  if (c->nranks == 1) {  // mpi_mod.hpp:1739-1746
    if (sendbuf && count && host)
      FTAR_CHECK_HIP(hipMemcpyAsync(recvbuf, sendbuf, count * esz, hipMemcpyHostToHost, stream));
    if (sendbuf && count && !host) return launch_copy(sendbuf, recvbuf, count * esz, stream);
    return FTAR_SUCCESS;
  }
  if (count == 0) return FTAR_SUCCESS;

  FTAR_RETURN_IF(resolve_call(c, topo_auto, count, esz, host != nullptr, &call));
  const Plan& plan = *call.plan;
  if (c->amax_cur && plan.own_block) {  // an amax call: this rank's block must have its root fold, where the
    bool root = false;                   // amax is taken -- never a silent 0
    for (const Stage& st : plan.stages)
      for (const ReduceItem& r : st.reduces) root |= r.root;
    if (!root) {
      set_error("this plan marks no root fold for the block this rank owns: no amax of it", __FILE__, __LINE__);
      return FTAR_ERR_UNSUPPORTED;
    }
  }
  switch (call.path) {
    case CallPath::PeerDevice:
      FTAR_RETURN_IF(grow_events(c, 5));
      return peer_allreduce(sendbuf, recvbuf, count, dt, op, plan, c, stream, call.peer_mode);
    case CallPath::PeerHostPipelined:
      // host buffers on a transport without p2p (a communicator bootstrapped over MPI with no RCCL,
      // ftar_comm_init_host): the read form piece by piece, H2D / exchange / D2H overlapped.  A bucket
      // of one piece per block gains nothing from it and takes the whole-bucket path, whose one
      // copy each way beats one per block (C1 through the MPI harness: 0.453 vs 0.487 ms)
      FTAR_RETURN_IF(grow_events(c, 5));
      return peer_allreduce_host(*host, count, dt, op, plan, c, stream, call.host_piece);
    case CallPath::PeerHostWhole:  // the write form (or FTAR_HOST_PEER_PIPELINE=0)
      return peer_allreduce_host_whole(*host, count, dt, op, plan, c, stream, call.peer_mode);
    case CallPath::Refused:  // a transport without p2p (ftar_comm_init_host): refused before anything moves
      set_error("this communicator has no point-to-point transfers: one-round plans in the peer-direct forms only "
                "(ftar_comm_set_peer_direct; staged forms and lonely ranks need RCCL)",
                __FILE__, __LINE__);
      return FTAR_ERR_UNSUPPORTED;
    case CallPath::Staged:
      break;
  }
  return staged_allreduce(sendbuf, recvbuf, count, dt, op, plan, call.ex.chunk, c, stream, host);
}

// One call on a communicator.  Calls share the communicator's scratch, staging
// and exchange buffers; the internal streams join the caller's stream at entry,
// so calls on ONE stream are ordered by it.  A call on another stream than the
// previous call's first waits for that call's completion marker (recorded on
// its stream after every internal stream joined it), so its transfers cannot
// overwrite scratch the previous call's reduces are still reading.
// Serial capture: a captured call issues everything on the caller's stream (FTAR_CAPTURE_SERIAL=1 / 0;
// default on when the loaded HIP runtime is older than 7.2).  torch 2.10 bundles HIP 7.0, whose
// hipStreamEndCapture dies (SIGSEGV, unbounded recursion) on the graph the forked comm/reduce streams and
// their per-piece cross waits leave, while 7.2 captures it; a chain in issue order keeps every
// dependency and gives up only the comm/reduce overlap inside the graph.
bool serial_capture() {
  static const bool on = [] {
    if (const char* e = getenv("FTAR_CAPTURE_SERIAL")) return *e != '0';
    int v = 0;
    return hipRuntimeGetVersion(&v) != hipSuccess || v < 70200000;  // major*1e7 + minor*1e5 + patch
  }();
  return on;
}

// argument checks the C entry points share (capi.cpp, engine_api.cpp)
ftar_status_t check_fold_shape(const int* shape, int nlevels, int k) {
  if (nlevels < 0 || nlevels > kMaxFoldLevels || (nlevels > 0 && !shape)) return FTAR_ERR_INVALID_ARG;
  if (nlevels > 1) {
    long long prod = 1;
    for (int l = 0; l < nlevels; ++l) {
      if (shape[l] < 1) return FTAR_ERR_INVALID_ARG;
      prod *= shape[l];
    }
    if (prod != k) return FTAR_ERR_INVALID_ARG;
  }
  return FTAR_SUCCESS;
}
ftar_status_t amax_supported(ftar_dtype_t dt, ftar_op_t op) {
  if ((op == FTAR_SUM || op == FTAR_AVG) && dtype_has_amax(dt)) return FTAR_SUCCESS;
  set_error("the amax entry points take SUM and AVG of f32, bf16, f16, f8e4m3 and f8e5m2", __FILE__, __LINE__);
  return FTAR_ERR_UNSUPPORTED;
}

namespace {
// one call with the communicator's lock held and its device current
ftar_status_t allreduce_held(const void* sendbuf, void* recvbuf, size_t count, ftar_dtype_t dt, ftar_op_t op,
                             const ftar_topo_t* topo, ftar_comm* c, hipStream_t stream, const HostIO* host) {
  // under capture the graph's own dependencies order its replays: an event recorded outside the capture
  // is not waited on inside it, nor is the marker re-recorded by a captured call
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  FTAR_CHECK_HIP(hipStreamIsCapturing(stream, &cs));
  const bool capturing = cs != hipStreamCaptureStatusNone;
  if (capturing && !c->tp->async_p2p() && c->nranks > 1) {  // its barriers synchronise the host
    set_error("a host-bootstrapped communicator cannot run under stream capture (its barriers synchronise the host)",
              __FILE__, __LINE__);
    return FTAR_ERR_UNSUPPORTED;
  }
  if (!capturing && c->done_recorded && c->done_stream != stream)
    FTAR_CHECK_HIP(hipStreamWaitEvent(stream, c->done_ev, 0));
  c->capturing = capturing;
  // serial capture: every internal stream is the caller's for this call, so the captured graph is one
  // chain in issue order (every wait refers to an event recorded earlier in that order, so the chain keeps
  // every dependency; the comm/reduce overlap is given up inside the graph)
  const bool serial = capturing && (serial_capture() || c->tp->capture_serially());
  if (host) FTAR_RETURN_IF(ensure_host_streams(c));
  hipStream_t saved[4] = {c->comm_s, c->red_s, c->h2d_s, c->d2h_s};
  if (serial) c->comm_s = c->red_s = c->h2d_s = c->d2h_s = stream;
  c->serial = serial;
  const ftar_status_t st = allreduce_locked(sendbuf, recvbuf, count, dt, op, topo, c, stream, host);
  if (serial) c->comm_s = saved[0], c->red_s = saved[1], c->h2d_s = saved[2], c->d2h_s = saved[3];
  c->serial = false;
  c->capturing = false;
  if (st == FTAR_SUCCESS && !capturing) {
    FTAR_CHECK_HIP(hipEventRecord(c->done_ev, stream));
    c->done_stream = stream;
    c->done_recorded = true;
  }
  return st;
}
}  // namespace

ftar_status_t allreduce(const void* sendbuf, void* recvbuf, size_t count, ftar_dtype_t dt, ftar_op_t op,
                        const ftar_topo_t* topo, ftar_comm* c, hipStream_t stream, const HostIO* host) {
  if (!c) return FTAR_ERR_INVALID_ARG;
  if (!dtype_op_supported(dt, op)) return FTAR_ERR_UNSUPPORTED;
  if (!recvbuf) {  // MPI allows null buffers with count 0 (e.g. an empty pinned tensor): nothing to do
    if (count) set_error("recvbuf is NULL", __FILE__, __LINE__);
    return count ? FTAR_ERR_INVALID_ARG : FTAR_SUCCESS;
  }
  std::lock_guard<std::mutex> g(c->mu);
  FTAR_CHECK_HIP(hipSetDevice(c->device));
  return allreduce_held(sendbuf, recvbuf, count, dt, op, topo, c, stream, host);
}

// The AllReduce and the amax of its result (ftar.h), all on `stream`: zero this rank's word; the unchanged
// AllReduce, whose root folds max the |stored value| keys of this rank's block into it (fold_op, the amax
// finish of reduce_impl.h); a second, P-element AllReduce of the ranks' words -- rank r's in slot r, zeros
// elsewhere, so no block is empty -- as MAX on FTAR_INT32: the key of a non-negative float is its bit pattern, a
// NAN's sorts above every number, and the integer MAX is exact on every topology and form; then one k = P fold
// of the slots into the caller's word.  The execution model prices neither extra step.
ftar_status_t allreduce_amax(const void* sendbuf, void* recvbuf, size_t count, ftar_dtype_t dt, ftar_op_t op,
                             const ftar_topo_t* topo, ftar_comm* c, float* amax, hipStream_t stream) {
  FTAR_RETURN_IF(amax_supported(dt, op));
  if (!amax || (reinterpret_cast<uintptr_t>(amax) & 3) || (!recvbuf && count)) {
    set_error(!amax ? "amax is NULL" : recvbuf ? "amax is not 4-byte aligned" : "recvbuf is NULL", __FILE__, __LINE__);
    return FTAR_ERR_INVALID_ARG;
  }
  if (!c) return FTAR_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  FTAR_CHECK_HIP(hipSetDevice(c->device));
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  FTAR_CHECK_HIP(hipStreamIsCapturing(stream, &cs));
  if (cs != hipStreamCaptureStatusNone) {
    set_error("ftar_allreduce_amax does not run under stream capture yet (ftar_reduce_amax and ftar_allreduce do)",
              __FILE__, __LINE__);
    return FTAR_ERR_UNSUPPORTED;
  }
  const size_t P = (size_t)c->nranks;
  unsigned* const word = c->amax_buf;
  unsigned* const slots = c->amax_buf + 1;
  if (count == 0) {  // nothing stored: +0.0
    FTAR_CHECK_HIP(hipMemsetAsync(amax, 0, sizeof(float), stream));
    return FTAR_SUCCESS;
  }
  // The word and the slots are the communicator's, like its scratch: a call on another stream than the previous
  // call's waits for that call's completion marker before it zeroes them (allreduce_held's rule, applied before
  // this call's first write), and the marker is recorded again below, after this call's last read of them.
  if (c->done_recorded && c->done_stream != stream) FTAR_CHECK_HIP(hipStreamWaitEvent(stream, c->done_ev, 0));
  auto done = [&]() -> ftar_status_t {
    FTAR_CHECK_HIP(hipEventRecord(c->done_ev, stream));
    c->done_stream = stream;
    c->done_recorded = true;
    return FTAR_SUCCESS;
  };
  FTAR_CHECK_HIP(hipMemsetAsync(c->amax_buf, 0, (1 + P) * sizeof(unsigned), stream));
  c->amax_cur = word;
  ftar_status_t st = allreduce_held(sendbuf, recvbuf, count, dt, op, topo, c, stream, nullptr);
  c->amax_cur = nullptr;
  if (st != FTAR_SUCCESS) {
    (void)done();  // the memset is enqueued: a later call on another stream still orders behind it
    return st;
  }
  if (P == 1) {
    FTAR_CHECK_HIP(hipMemcpyAsync(amax, word, sizeof(unsigned), hipMemcpyDeviceToDevice, stream));
    return done();
  }
  FTAR_CHECK_HIP(hipMemcpyAsync(slots + c->rank, word, sizeof(unsigned), hipMemcpyDeviceToDevice, stream));
  // the second round is internal: ftar_comm_last_exec and the phase marks keep describing the bucket's AllReduce
  const ftar_exec_t bucket_exec = c->last_exec;
  const size_t bucket_marks = c->nmarks;
  const bool timing = c->phase_timing;
  c->phase_timing = false;
  st = allreduce_held(nullptr, slots, P, FTAR_INT32, FTAR_MAX, topo, c, stream, nullptr);
  c->phase_timing = timing;
  c->nmarks = bucket_marks;
  c->last_exec = bucket_exec;
  if (st != FTAR_SUCCESS) {
    (void)done();
    return st;
  }
  std::vector<const void*> srcs;
  FoldCall f;
  f.dst = amax; f.count = 1; f.dt = FTAR_INT32; f.op = FTAR_MAX; f.stream = stream;
  for (size_t lo = 0; lo < P; lo += FTAR_MAX_K - 1) {  // (more ranks than one fold has sources: in turns)
    srcs.clear();
    if (lo) srcs.push_back(amax);
    for (size_t j = lo; j < std::min(P, lo + FTAR_MAX_K - 1); ++j) srcs.push_back(slots + j);
    f.srcs = srcs.data(); f.k = (int)srcs.size();
    FTAR_RETURN_IF(launch_reduce(f));
  }
  return done();
}

}  // namespace ftar

// ============================================================================
// C ABI: communicators and AllReduce
// ============================================================================
