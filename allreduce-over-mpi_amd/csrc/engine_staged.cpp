// The staged two-stream executor (engine_state.h; the pipeline itself is described at the top of engine.cpp):
// a plan's stages piece by piece, transfers on the comm stream and folds on the reduce stream, for device
// buffers and, through a device staging buffer, for host buffers on a transport with point-to-point transfers.
#include <algorithm>
#include <string>
#include <utility>

#include "engine_state.h"

namespace ftar {

namespace {
// Host mode pieces (0 = auto): 16 MiB per block, at least split/64 (bounds the
// number of copies for huge buckets).  4 MiB device->host copies run at only
// ~33 GB/s; larger pieces lengthen the pipeline's fill and drain (one piece of
// every block each).  16 MiB was the best or near-best size in every sweep
// (profiles/r01/host/): 8 pieces per block at P = 8 x 1 GiB.
size_t auto_host_chunk(size_t split_bytes) { return std::max<size_t>(16u << 20, split_bytes / 64); }

// Per-stage dependency facts of a plan: does it move / reduce / receive into
// scratch, the latest reducing stage before it (its data), and in the
// stage-major order the last reader of the scratch half it receives into.
struct StageFacts {
  std::vector<char> moves, reduces, to_scratch;
  std::vector<long> prev_red, war;
  explicit StageFacts(const Plan& plan) {
    const size_t nst = plan.stages.size();
    moves.assign(nst, 0);
    reduces.assign(nst, 0);
    to_scratch.assign(nst, 0);
    prev_red.assign(nst, -1);
    war.assign(nst, -1);
    long last = -1, owner[2] = {-1, -1};
    for (size_t s = 0; s < nst; ++s) {
      const Stage& st = plan.stages[s];
      moves[s] = !st.sends.empty() || !st.recvs.empty();
      reduces[s] = !st.reduces.empty();
      for (const Transfer& x : st.recvs) to_scratch[s] |= x.buf == BUF_SCRATCH;
      prev_red[s] = last;
      war[s] = to_scratch[s] ? owner[s % 2] : -1;
      if (reduces[s]) {
        last = (long)s;
        if (to_scratch[s]) owner[s % 2] = (long)s;
      }
    }
  }
};

// Skewed execution gives every stage its own scratch region: delta[s] moves a
// stage's scratch offsets from its alternating half to that region.  Returns
// the scratch elements needed.
size_t per_stage_scratch(const Plan& plan, std::vector<long>* delta) {
  const size_t nst = plan.stages.size();
  delta->assign(nst, 0);
  size_t base = 0;
  for (size_t s = 0; s < nst; ++s) {
    const size_t half_base = (s % 2) * plan.scratch_half;
    size_t used = 0;
    for (const Transfer& x : plan.stages[s].recvs)
      if (x.buf == BUF_SCRATCH) used = std::max(used, x.off - half_base + x.len);
    (*delta)[s] = (long)base - (long)half_base;
    base += used;
  }
  return base;
}

// Order of the (stage, piece) steps, identical on every rank.  Stage-major, or
// skewed: stage s+1 trails stage s by one piece.
std::vector<std::pair<size_t, size_t>> step_order(size_t nst, size_t nchunks, bool skew) {
  std::vector<std::pair<size_t, size_t>> order;
  order.reserve(nst * nchunks);
  if (!skew) {
    for (size_t s = 0; s < nst; ++s)
      for (size_t k = 0; k < nchunks; ++k) order.emplace_back(s, k);
  } else {
    for (size_t tt = 0; tt < nchunks + nst - 1; ++tt)
      for (size_t s = 0; s < nst && s <= tt; ++s)
        if (tt - s < nchunks) order.emplace_back(s, tt - s);
  }
  return order;
}

}  // namespace

ftar_status_t staged_allreduce(const void* sendbuf, void* recvbuf, size_t count, ftar_dtype_t dt, ftar_op_t op,
                               const Plan& plan, size_t model_chunk, ftar_comm* c, hipStream_t stream,
                               const HostIO* host) {
  const size_t esz = dtype_size(dt), nst = plan.stages.size();
  // AVG: SUM, scaled by 1 / P on the plan's root items; an amax call: they max into the call's word too
  const FoldOp fo = fold_op(op, dt, c->nranks, c->amax_cur);
  // Host mode: the buffers are in host memory and move through a device
  // staging buffer, piece by piece, so H2D (PCIe in), the exchange, and D2H
  // (PCIe out) run at the same time.  Every src/dst transfer and reduce of a
  // plan covers whole blocks from their start (tests/test_plan.py), so piece
  // k of every stage touches exactly piece k of each block: the same bytes,
  // the same partition, the same bits as the device path.
  // the piece: fixed, or the model's (0 = whole blocks)
  size_t chunk_bytes = c->chunk_bytes ? c->chunk_bytes : model_chunk ? model_chunk : plan.split * esz;
  if (host) {
    chunk_bytes = c->host_chunk_bytes ? c->host_chunk_bytes : auto_host_chunk(plan.split * esz);
    c->last_exec.chunk_bytes = std::max<size_t>(64, (chunk_bytes / esz) & ~size_t(63)) * esz;  // the piece run
    if (count * esz > c->staging_bytes) FTAR_RETURN_IF(refuse_growth_under_capture(c, "the staging buffer"));
    FTAR_RETURN_IF(ensure_buffer(&c->staging, &c->staging_bytes, count * esz, {c->h2d_s, c->comm_s, c->red_s, c->d2h_s}));
    sendbuf = nullptr;
    recvbuf = c->staging;
  }
  const size_t chunk = std::max<size_t>(64, (chunk_bytes / esz) & ~size_t(63));
  const size_t nchunks = std::max<size_t>(1, (plan.split + chunk - 1) / chunk);
  const StageFacts f(plan);
  const std::vector<char>&moves = f.moves, &reduces = f.reduces;
  const std::vector<long>&prev_red = f.prev_red, &war = f.war;
  // Device: stage-major.  Host: skewed, so the all-gather of piece k (and its
  // D2H) runs while later pieces are still coming in over PCIe; skewed steps
  // of stages two apart may overlap in time, so every stage gets its own
  // scratch region instead of alternating halves.
  const bool skew = host != nullptr;
  std::vector<long> delta(nst, 0);
  const size_t scratch_elems = skew ? per_stage_scratch(plan, &delta) : 2 * plan.scratch_half;
  if (scratch_elems * esz > c->scratch_bytes) {
    FTAR_RETURN_IF(refuse_growth_under_capture(c, "the scratch buffer"));
    if (c->scratch_rccl) {  // the old scratch is about to be freed: drop its RCCL registration first
      FTAR_CHECK_HIP(hipStreamSynchronize(c->comm_s));
      FTAR_CHECK_HIP(hipStreamSynchronize(c->red_s));
      c->tp->rccl_deregister(c->scratch_rccl);
      c->scratch_rccl = nullptr;
    }
  }
  FTAR_RETURN_IF(ensure_buffer(&c->scratch, &c->scratch_bytes, scratch_elems * esz, {c->comm_s, c->red_s}));
  if (c->rccl_reg && !c->scratch_rccl && c->scratch && !c->capturing)
    c->scratch_rccl = c->tp->rccl_register(c->scratch, c->scratch_bytes);
  const std::vector<std::pair<size_t, size_t>> order = step_order(nst, nchunks, skew);

  FTAR_RETURN_IF(grow_events(c, 2 * nst * nchunks + 2 * nchunks + 5));
  hipEvent_t* ev = c->events.data();
  auto ev_x = [&](size_t s, size_t k) { return ev[5 + (s * nchunks + k) * 2]; };
  auto ev_r = [&](size_t s, size_t k) { return ev[5 + (s * nchunks + k) * 2 + 1]; };
  auto ev_h = [&](size_t k) { return ev[5 + 2 * nst * nchunks + 2 * k]; };
  auto ev_d = [&](size_t k) { return ev[5 + 2 * nst * nchunks + 2 * k + 1]; };

  char* bufs[3] = {static_cast<char*>(const_cast<void*>(sendbuf ? sendbuf : recvbuf)), static_cast<char*>(recvbuf),
                   static_cast<char*>(c->scratch)};
  Transport* tp = c->tp.get();
  const size_t P = (size_t)c->nranks, split = plan.split;

  // ---- Host mode, all of it: five hooks the step loop calls; none of them does anything for device buffers.
  // The pieces go in, in order, on their own stream, issued kHostLookahead pieces ahead of the
  // steps that read them rather than all up front.  The copy stream then runs ahead of the exchange by
  // that many pieces either way, and a stream that shares its hardware queue with it (8 streams of two
  // in-process ranks on HIP's 4 queues, or a caller's own streams) waits behind those few pieces, not
  // behind the whole bucket: with every piece issued first, two ranks on one GPU started the exchange only
  // once the last piece was in, and H2D and D2H never overlapped (profiles/r05/host_local/).
  size_t h2d_issued = 0;
  auto host_lookahead = [&](size_t upto) -> ftar_status_t {  // H2D of pieces [h2d_issued, upto] of every block
    for (; host && h2d_issued <= upto && h2d_issued < nchunks; ++h2d_issued) {
      const size_t k = h2d_issued;
      FTAR_RETURN_IF(for_piece(P, split, chunk, count, k, [&](size_t lo, size_t n) -> ftar_status_t {
        FTAR_CHECK_HIP(hipMemcpyAsync(bufs[BUF_DST] + lo * esz, host->src + lo * esz, n * esz,
                                      hipMemcpyHostToDevice, c->h2d_s));
        return FTAR_SUCCESS;
      }));
      FTAR_CHECK_HIP(hipEventRecord(ev_h(k), c->h2d_s));
    }
    return FTAR_SUCCESS;
  };
  auto host_fork = [&]() -> ftar_status_t {  // the copy streams join the call, the first pieces go in
    if (!host) return FTAR_SUCCESS;
    FTAR_CHECK_HIP(hipStreamWaitEvent(c->h2d_s, ev[0], 0));
    FTAR_CHECK_HIP(hipStreamWaitEvent(c->d2h_s, ev[0], 0));
    return host_lookahead(kHostLookahead);
  };
  std::vector<char> comm_has_input(host ? nchunks : 0), red_has_input(host ? nchunks : 0);
  auto host_input = [&](hipStream_t s, std::vector<char>& has, size_t k) -> ftar_status_t {  // s: once piece k is in
    if (!host || has[k]) return FTAR_SUCCESS;
    FTAR_CHECK_HIP(hipStreamWaitEvent(s, ev_h(k), 0));
    has[k] = 1;
    return FTAR_SUCCESS;
  };
  auto host_final = [&](size_t s, size_t k) -> ftar_status_t {  // after step (s, k): D2H of a piece that is final
    if (!host || s != nst - 1) return FTAR_SUCCESS;  // final everywhere: out over PCIe while later pieces come in
    FTAR_CHECK_HIP(hipEventRecord(ev_d(k), reduces[s] ? c->red_s : c->comm_s));
    if (reduces[s]) FTAR_CHECK_HIP(hipStreamWaitEvent(c->d2h_s, ev_x(s, k), 0));
    else if (prev_red[s] >= 0)  // a rank idle in the last stage: its block's final fold
      FTAR_CHECK_HIP(hipStreamWaitEvent(c->d2h_s, ev_r((size_t)prev_red[s], k), 0));
    FTAR_CHECK_HIP(hipStreamWaitEvent(c->d2h_s, ev_d(k), 0));
    return for_piece(P, split, chunk, count, k, [&](size_t lo, size_t n) -> ftar_status_t {
      FTAR_CHECK_HIP(hipMemcpyAsync(host->dst + lo * esz, bufs[BUF_DST] + lo * esz, n * esz,
                                    hipMemcpyDeviceToHost, c->d2h_s));
      return FTAR_SUCCESS;
    });
  };
  auto host_join = [&]() -> ftar_status_t {
    return host ? join_streams(stream, {{ev[3], c->h2d_s}, {ev[4], c->d2h_s}}) : FTAR_SUCCESS;
  };

  FTAR_RETURN_IF(fork_streams(stream, ev[0], {c->comm_s, c->red_s}));
  c->nmarks = 0;
  FTAR_RETURN_IF(mark(c, "start", c->comm_s));
  FTAR_RETURN_IF(host_fork());
  std::vector<const void*> srcs;
  auto sbuf = [&](int buf, size_t off, size_t s) -> char* {
    return bufs[buf] + (buf == BUF_SCRATCH ? (size_t)((long)off + delta[s]) : off) * esz;
  };
  for (const auto& step : order) {
    const size_t s = step.first, k = step.second, lo = k * chunk;
    const Stage& st = plan.stages[s];
    FTAR_RETURN_IF(host_lookahead(k + kHostLookahead));
    if (moves[s]) {
      FTAR_RETURN_IF(host_input(c->comm_s, comm_has_input, k));
      // WAR on the scratch half this stage receives into (stage-major only):
      // every reduce that read it (stage s-2, or earlier when stages in between
      // were empty) must be done.  When stage s-1 reduced, its piece-0 event
      // already implies this (the reduce stream runs in order), so the wait is
      // free; it matters when s-1 was empty.
      if (!skew && k == 0 && war[s] >= 0)
        FTAR_CHECK_HIP(hipStreamWaitEvent(c->comm_s, ev_r((size_t)war[s], nchunks - 1), 0));
      if (prev_red[s] >= 0) FTAR_CHECK_HIP(hipStreamWaitEvent(c->comm_s, ev_r((size_t)prev_red[s], k), 0));
      FTAR_RETURN_IF(tp->group_start());
      for (const Transfer& x : st.sends)
        if (x.len > lo)
          FTAR_RETURN_IF(tp->send(sbuf(x.buf, x.off + lo, s), std::min(chunk, x.len - lo) * esz, x.peer, c->comm_s));
      for (const Transfer& x : st.recvs)
        if (x.len > lo)
          FTAR_RETURN_IF(tp->recv(sbuf(x.buf, x.off + lo, s), std::min(chunk, x.len - lo) * esz, x.peer, c->comm_s));
      FTAR_RETURN_IF(tp->group_end());
    }
    if (reduces[s]) {
      FTAR_CHECK_HIP(hipEventRecord(ev_x(s, k), c->comm_s));
      FTAR_CHECK_HIP(hipStreamWaitEvent(c->red_s, ev_x(s, k), 0));
      FTAR_RETURN_IF(host_input(c->red_s, red_has_input, k));
      for (const ReduceItem& r : st.reduces) {
        if (r.len <= lo) continue;
        srcs.clear();
        for (const Operand& o : r.srcs) srcs.push_back(sbuf(o.buf, o.off + lo, s));
        FoldCall f;
        f.srcs = srcs.data(); f.k = (int)srcs.size(); f.dst = bufs[BUF_DST] + (r.off + lo) * esz;
        f.count = std::min(chunk, r.len - lo); f.dt = dt; f.op = fo.op; f.stream = c->red_s;
        f.round_each = r.round_each; f.shape = r.shape.data(); f.nlevels = (int)r.shape.size();
        f.scale = fo.scale(r.root); f.amax = fo.amax(r.root);
        FTAR_RETURN_IF(launch_reduce(f));
      }
      FTAR_CHECK_HIP(hipEventRecord(ev_r(s, k), c->red_s));
    }
    if (c->phase_timing && !skew && k == nchunks - 1) {  // stage-major: the stage's last piece
      if (moves[s]) FTAR_RETURN_IF(mark(c, "stage " + std::to_string(s) + " moved", c->comm_s));
      if (reduces[s]) FTAR_RETURN_IF(mark(c, "stage " + std::to_string(s) + " reduced", c->red_s));
    }
    FTAR_RETURN_IF(host_final(s, k));
  }
  FTAR_RETURN_IF(host_lookahead(nchunks - 1));  // (every piece is read by a step; kept for safety)
  if (plan.allgather == FTAR_AG_COLLECTIVE) {  // the whole all-gather phase as one collective, in place
    const long last_red = nst ? (reduces[nst - 1] ? (long)nst - 1 : prev_red[nst - 1]) : -1;
    if (last_red >= 0) FTAR_CHECK_HIP(hipStreamWaitEvent(c->comm_s, ev_r((size_t)last_red, nchunks - 1), 0));
    FTAR_RETURN_IF(tp->allgather(bufs[BUF_DST] + (size_t)c->rank * plan.split * esz, bufs[BUF_DST], plan.split * esz,
                                 c->rank, c->nranks, c->comm_s));
    FTAR_RETURN_IF(mark(c, "collective all-gather", c->comm_s));
  }
  FTAR_RETURN_IF(tp->before_join());
  FTAR_RETURN_IF(join_streams(stream, {{ev[1], c->comm_s}, {ev[2], c->red_s}}));
  return host_join();
}

}  // namespace ftar
