// The in-process transport: N ranks inside one process (one host thread per rank) and the hub they meet in.
//
// The receiver enqueues a device copy from the sender's
// buffer on its own stream, ordered after the sender's
// "ready" event; the sender's stream then waits for the
// receiver's "copied" event.  Same per-pair FIFO matching,
// same stream semantics as RCCL p2p, so the engine code
// above it is identical; used to run multi-rank schedules
// on a single GPU (tests) and in single-process groups.
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>

#include "ftar_internal.h"

namespace ftar {

namespace {
thread_local bool t_issue_held = false;  // this thread holds its group's issue lock (capture)
}

struct LocalHub {
  // Per-message and barrier events are recycled through a pool, never
  // destroyed before the hub: a stream capture may still refer to an event
  // after both sides dropped the message.
  // A pooled event shared by the messages of one flush: the sends of a flush on one stream share their
  // data-ready event, the receives of a flush on one stream their copies-done event (one record each
  // instead of one per message); the last holder gives it back to the pool.
  using Ev = std::shared_ptr<hipEvent_t>;
  struct Posted {
    const void* buf;
    size_t bytes;
    Ev ready;     // sender-side data ready
    Ev done;      // receiver-side copy finished (set by the receiver)
    bool taken = false;
    int device = -1;  // the sender's device
    int sender = -1;
  };
  ftar_status_t take_shared(Ev* out) {
    Ev e(new hipEvent_t(nullptr), [this](hipEvent_t* p) {
      if (*p) give_event(*p);
      delete p;
    });
    FTAR_RETURN_IF(take_event(e.get()));
    *out = std::move(e);
    return FTAR_SUCCESS;
  }
  // During a capture (this thread holds the issue lock) every record gets a
  // fresh event and used ones retire until the next uncaptured use: an event
  // re-recorded inside one capture -- on another rank's stream after a peer
  // waited on it -- made hipStreamEndCapture recurse without end
  // (tools/capture/, profiles/r02/capture/).
  ftar_status_t take_event(hipEvent_t* e) {
    {
      std::lock_guard<std::mutex> g(pool_mu);
      if (!t_issue_held && !retired.empty()) {
        pool.insert(pool.end(), retired.begin(), retired.end());
        retired.clear();
      }
      if (!t_issue_held && !pool.empty()) {
        *e = pool.back();
        pool.pop_back();
        return FTAR_SUCCESS;
      }
    }
    FTAR_CHECK_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return FTAR_SUCCESS;
  }
  void give_event(hipEvent_t e) {
    std::lock_guard<std::mutex> g(pool_mu);
    (t_issue_held ? retired : pool).push_back(e);
  }
  ~LocalHub() {
    // the last rendezvous rounds and any undelivered messages still hold pooled events whose deleters give
    // them back here: release them while the pool is alive, then destroy the pool (a barrier's round left
    // in `done` was given back into the destroyed pool after it, a double free on destroying a group whose
    // last call was a peer form)
    done.reset();
    pending.reset();
    wire.clear();
    for (hipEvent_t e : pool) hip_ignore(hipEventDestroy(e));
    for (hipEvent_t e : retired) hip_ignore(hipEventDestroy(e));
    pool.clear();
    retired.clear();
  }
  // Rank `rank` waits on its own condition variable (a message for it, its message taken, a rendezvous
  // complete), so a notification wakes the one thread it concerns rather than every rank's.  The wait lets
  // the other ranks' threads issue meanwhile when this one holds the issue lock (lock order: issue before mu).
  template <class Pred>
  bool wait(std::unique_lock<std::mutex>& g, int rank, Pred pred) {
    std::condition_variable& cv = rcv[rank];
    if (!t_issue_held) return cv.wait_for(g, std::chrono::seconds(120), pred);
    if (pred()) return true;
    g.unlock();
    issue.unlock();
    g.lock();
    const bool ok = cv.wait_for(g, std::chrono::seconds(120), pred);
    g.unlock();
    issue.lock();
    g.lock();
    return ok;
  }
  // every rank's value of one rendezvous (barriers, peer pointers)
  struct Round {
    std::vector<const void*> ptr;
    std::vector<std::shared_ptr<hipEvent_t>> ev;
  };
  std::shared_ptr<Round> fresh_round() const {
    auto r = std::make_shared<Round>();
    r->ptr.resize(nranks);
    r->ev.resize(nranks);
    return r;
  }
  void notify(int rank) { rcv[rank].notify_all(); }
  // After any transport failure the group is unusable: messages of the failed call may still
  // sit in `wire` and a failed sender's buffer may still be read by copies enqueued for it, so a later call
  // could pair a receive with a stale message.  fail() records the first failure and wakes every waiter;
  // every later operation of every rank is refused (destroy the group and create a new one).
  void fail(const std::string& why) {
    {
      std::lock_guard<std::mutex> g(mu);
      if (broken.empty()) broken = why.empty() ? std::string("a transport failure") : why;
    }
    for (int q = 0; q < nranks; ++q) rcv[q].notify_all();
  }
  ftar_status_t usable() {
    std::string why;
    {
      std::lock_guard<std::mutex> g(mu);
      why = broken;
    }
    if (why.empty()) return FTAR_SUCCESS;
    set_error("local transport: this group failed in an earlier call (" + why +
                  "); destroy it and create a new one",
              __FILE__, __LINE__);
    return FTAR_ERR_INTERNAL;
  }
  // whether kernels on device `dev` may read device `peer`'s memory (ftar_comm_init_local enables peer
  // access between every pair that supports it), cached per pair
  bool can_reach(int dev, int peer) {
    std::lock_guard<std::mutex> g(pool_mu);
    auto it = reach.find({dev, peer});
    if (it != reach.end()) return it->second;
    int can = 0;
    const bool ok = hipDeviceCanAccessPeer(&can, dev, peer) == hipSuccess && can;
    reach[{dev, peer}] = ok;
    return ok;
  }
  explicit LocalHub(int n) : nranks(n), rcv(new std::condition_variable[n]), pending(fresh_round()) {}
  // Host-side all-gather of one (pointer, event) per rank.  A generation
  // completes only when every rank arrived, so the finished Round cannot be
  // replaced before each of its ranks has taken it.
  ftar_status_t rendezvous(int rank, const void* p, std::shared_ptr<hipEvent_t> e, std::shared_ptr<Round>* out) {
    std::unique_lock<std::mutex> g(mu);
    const long my_gen = gen;
    pending->ptr[rank] = p;
    pending->ev[rank] = std::move(e);
    if (++arrived == nranks) {
      done = pending;
      pending = fresh_round();
      arrived = 0;
      ++gen;
      for (int q = 0; q < nranks; ++q) rcv[q].notify_all();
    } else if (!wait(g, rank, [&] { return gen != my_gen || !broken.empty(); })) {
      set_error("local transport: rendezvous timed out", __FILE__, __LINE__);
      return FTAR_ERR_TIMEOUT;
    } else if (gen == my_gen) {
      set_error("local transport: another rank failed during a rendezvous (" + broken + ")", __FILE__, __LINE__);
      return FTAR_ERR_INTERNAL;
    }
    *out = done;
    return FTAR_SUCCESS;
  }
  int nranks;
  std::mutex mu;
  std::unique_ptr<std::condition_variable[]> rcv;  // one per rank
  std::map<std::pair<int, int>, std::deque<std::shared_ptr<Posted>>> wire;  // (from, to)
  std::shared_ptr<Round> pending, done;
  int arrived = 0;
  long gen = 0;
  std::string broken;  // the first failure (under mu); non-empty: every later operation is refused
  std::mutex issue;  // capture of the group: one issuing thread at a time
  std::mutex pool_mu;
  std::vector<hipEvent_t> pool, retired;
  std::map<std::pair<int, int>, bool> reach;  // can_reach, under pool_mu
};

std::shared_ptr<LocalHub> make_local_hub(int nranks) { return std::make_shared<LocalHub>(nranks); }

namespace {

// FTAR_LOCAL_COPY, read once per process: how a receive copies (LocalTransport::copy_for)
enum CopyMode { kCopyRuntime = 0, kCopyDefault = 1, kCopyGather = 2 };
CopyMode local_copy_mode() {
  static const CopyMode mode = [] {
    const char* e = getenv("FTAR_LOCAL_COPY");
    return e && !strcmp(e, "runtime") ? kCopyRuntime : e && !strcmp(e, "gather") ? kCopyGather : kCopyDefault;
  }();
  return mode;
}

// the entry of stream `st` in a per-stream list of one flush, made on first use
template <class T>
T* slot_for(std::vector<std::pair<hipStream_t, T>>& v, hipStream_t st) {
  for (auto& x : v)
    if (x.first == st) return &x.second;
  v.emplace_back(st, T());
  return &v.back().second;
}

class LocalTransport final : public Transport {
  using Ev = LocalHub::Ev;
  using Posted = LocalHub::Posted;
  struct Op {
    bool is_send;
    void* buf;
    size_t bytes;
    int peer;
    hipStream_t s;
  };
  // One flush: a group's sends and receives, issued together.
  struct Flush {
    int dev = -1;                                      // this rank's device
    std::vector<std::pair<hipStream_t, Ev>> ready;     // per sending stream: its data-ready event, recorded once
    std::vector<std::pair<hipStream_t, Ev>> done;      // per receiving stream: its copies-done event, recorded once
    std::vector<std::shared_ptr<Posted>> mine;         // the sends, in posting order
    std::vector<std::pair<std::shared_ptr<Posted>, hipStream_t>> got;    // every message taken, and its receiving stream
    std::vector<std::pair<hipStream_t, hipEvent_t>> waited;              // (stream, event) already waited on
    std::vector<std::pair<hipStream_t, std::vector<Segment>>> gathers;   // batched receives per stream
  };
  enum class Copy { kGather, kKernel, kRuntime };

 public:
  LocalTransport(std::shared_ptr<LocalHub> h, int rank) : hub_(std::move(h)), rank_(rank) {}
  ftar_status_t group_start() override {
    ++depth_;
    return FTAR_SUCCESS;
  }
  ftar_status_t send(const void* buf, size_t bytes, int peer, hipStream_t s) override {
    ops_.push_back({true, const_cast<void*>(buf), bytes, peer, s});
    return depth_ ? FTAR_SUCCESS : flush();
  }
  ftar_status_t recv(void* buf, size_t bytes, int peer, hipStream_t s) override {
    ops_.push_back({false, buf, bytes, peer, s});
    return depth_ ? FTAR_SUCCESS : flush();
  }
  ftar_status_t group_end() override {
    if (depth_ <= 0) return FTAR_ERR_INVALID_ARG;
    if (--depth_ == 0) return flush();
    return FTAR_SUCCESS;
  }
  const char* name() const override { return "local"; }
  bool capture_serially() const override { return true; }
  void capture_enter() override {
    hub_->issue.lock();
    t_issue_held = true;
  }
  void capture_leave() override {
    t_issue_held = false;
    hub_->issue.unlock();
  }
  ftar_status_t before_join() override {
    if (!t_issue_held) return FTAR_SUCCESS;
    return guarded([&] {
      std::shared_ptr<LocalHub::Round> r;
      return hub_->rendezvous(rank_, nullptr, nullptr, &r);
    });
  }
  ftar_status_t barrier(hipStream_t s) override {
    return guarded([&] { return barrier_impl(s); });
  }
  ftar_status_t map_peers(void* mine, int rank, int nranks, std::vector<char*>* peers) override {
    return guarded([&] { return map_peers_impl(mine, rank, nranks, peers); });
  }

 private:
  // refused once the group failed; a failure here breaks the group for every rank
  template <class F>
  ftar_status_t guarded(F&& fn) {
    FTAR_RETURN_IF(hub_->usable());
    const ftar_status_t st = fn();
    if (st != FTAR_SUCCESS) hub_->fail(last_error());
    return st;
  }
  // each rank's stream waits for every other rank's event recorded at the barrier
  ftar_status_t barrier_impl(hipStream_t s) {
    Ev e;
    FTAR_RETURN_IF(hub_->take_shared(&e));
    FTAR_CHECK_HIP(hipEventRecord(*e, s));
    std::shared_ptr<LocalHub::Round> r;
    FTAR_RETURN_IF(hub_->rendezvous(rank_, nullptr, e, &r));
    for (int q = 0; q < hub_->nranks; ++q)
      if (q != rank_) FTAR_CHECK_HIP(hipStreamWaitEvent(s, *r->ev[q], 0));
    return FTAR_SUCCESS;
  }
  // one address space: the peers' allocations are usable as they are
  ftar_status_t map_peers_impl(void* mine, int rank, int nranks, std::vector<char*>* peers) {
    (void)rank;
    std::shared_ptr<LocalHub::Round> r;
    FTAR_RETURN_IF(hub_->rendezvous(rank_, mine, nullptr, &r));
    peers->assign(nranks, nullptr);
    for (int q = 0; q < nranks; ++q) (*peers)[q] = static_cast<char*>(const_cast<void*>(r->ptr[q]));
    return FTAR_SUCCESS;
  }

  ftar_status_t flush() {
    std::vector<Op> ops;
    ops.swap(ops_);
    return guarded([&] { return flush_ops(ops); });
  }

  // A failure after the first message was taken goes through hand_back, so every sender whose message this
  // rank holds fails with it, at once, rather than waiting out the timeout.
  ftar_status_t flush_ops(std::vector<Op>& ops) {
    Flush f;
    FTAR_CHECK_HIP(hipGetDevice(&f.dev));
    FTAR_RETURN_IF(post_sends(ops, f));
    const ftar_status_t st = issue_receives(ops, f);
    FTAR_RETURN_IF(hand_back(f, st));
    return await_receivers(ops, f);
  }

  // 1. publish every send, with an event marking its data ready on the sender's stream (one per stream)
  ftar_status_t post_sends(const std::vector<Op>& ops, Flush& f) {
    for (auto& o : ops) {
      if (!o.is_send) continue;
      if (o.peer == rank_ || o.peer < 0 || o.peer >= hub_->nranks) return FTAR_ERR_INVALID_ARG;
      Ev* e = slot_for(f.ready, o.s);
      if (!*e) {
        FTAR_RETURN_IF(hub_->take_shared(e));
        FTAR_CHECK_HIP(hipEventRecord(**e, o.s));
      }
      auto p = std::make_shared<Posted>();
      p->buf = o.buf;
      p->bytes = o.bytes;
      p->ready = *e;
      p->device = f.dev;
      p->sender = rank_;
      f.mine.push_back(p);
      {
        std::lock_guard<std::mutex> g(hub_->mu);
        hub_->wire[{rank_, o.peer}].push_back(p);
      }
      hub_->notify(o.peer);
    }
    return FTAR_SUCCESS;
  }

  // 2. issue every receive in posting order (per-pair FIFO, like MPI/RCCL): wait for the sender's data,
  // copy; the first failure ends it (the caller hands back what was taken)
  ftar_status_t issue_receives(const std::vector<Op>& ops, Flush& f) {
    for (auto& o : ops) {
      if (o.is_send) continue;
      std::shared_ptr<Posted> p;
      FTAR_RETURN_IF(take(o, &p));
      f.got.emplace_back(p, o.s);
      FTAR_RETURN_IF(issue_receive(o, *p, f));
    }
    for (auto& g : f.gathers)
      for (size_t i = 0; i < g.second.size(); i += FTAR_MAX_K) {
        const int m = (int)std::min<size_t>(FTAR_MAX_K, g.second.size() - i);
        FTAR_RETURN_IF(launch_gather(g.second.data() + i, m, g.first));
      }
    return FTAR_SUCCESS;
  }

  // the next message from o.peer, waited for
  ftar_status_t take(const Op& o, std::shared_ptr<Posted>* p) {
    std::unique_lock<std::mutex> g(hub_->mu);
    auto& q = hub_->wire[{o.peer, rank_}];
    if (!hub_->wait(g, rank_, [&] { return !q.empty() || !hub_->broken.empty(); })) {
      g.unlock();
      set_error("local transport: no matching send from rank " + std::to_string(o.peer), __FILE__, __LINE__);
      return FTAR_ERR_TIMEOUT;
    }
    if (q.empty()) {
      const std::string why = hub_->broken;
      g.unlock();
      set_error("local transport: another rank failed (" + why + ")", __FILE__, __LINE__);
      return FTAR_ERR_INTERNAL;
    }
    *p = q.front();
    q.pop_front();
    return FTAR_SUCCESS;
  }

  // A receive from a rank on this device is ftar's own copy kernel, one launch per receive (launch_copy:
  // the LDS-staged copy when co-aligned): 5-6 % faster than the runtime's blit at the C4 bucket with 8
  // ranks on one GPU (profiles/r05/engine_local/ab2_*, 3 interleaved rounds); one launch per piece group
  // instead lost 2 % (it filled the GPU, and the folds stopped overlapping the copies).  The receives
  // from other devices this device can reach go into one multi-segment copy per stream, launched once
  // every one of them is waited for: its workgroups interleave the segments, so every peer's link
  // streams at once (one runtime copy after another would use one link at a time); without peer access
  // the runtime copies.  FTAR_LOCAL_COPY=runtime: the runtime's copy for every receive; =gather: the
  // multi-segment copy for every receive, same device included (the A/Bs, and the test of that path on
  // a one-GPU box).
  Copy copy_for(const Posted& p, int dev) {
    const CopyMode mode = local_copy_mode();
    if (mode == kCopyGather || (mode == kCopyDefault && p.device != dev && hub_->can_reach(dev, p.device)))
      return Copy::kGather;
    return mode == kCopyDefault && p.device == dev ? Copy::kKernel : Copy::kRuntime;
  }

  // one taken message on its receive's stream: after the sender's data-ready event (waited for once per
  // stream and event), the copy, or its segment in the stream's multi-segment copy
  ftar_status_t issue_receive(const Op& o, const Posted& p, Flush& f) {
    if (p.bytes != o.bytes) {
      set_error("local transport: message size mismatch", __FILE__, __LINE__);
      return FTAR_ERR_INTERNAL;
    }
    const std::pair<hipStream_t, hipEvent_t> w{o.s, *p.ready};
    if (std::find(f.waited.begin(), f.waited.end(), w) == f.waited.end()) {
      if (hipStreamWaitEvent(o.s, *p.ready, 0) != hipSuccess) {
        set_error("local transport: hipStreamWaitEvent failed", __FILE__, __LINE__);
        return FTAR_ERR_HIP;
      }
      f.waited.push_back(w);
    }
    if (!o.bytes) return FTAR_SUCCESS;
    switch (copy_for(p, f.dev)) {
      case Copy::kGather: slot_for(f.gathers, o.s)->push_back({p.buf, o.buf, o.bytes}); break;
      case Copy::kKernel: return launch_copy(p.buf, o.buf, o.bytes, o.s);
      case Copy::kRuntime:
        if (hipMemcpyAsync(o.buf, p.buf, o.bytes, hipMemcpyDeviceToDevice, o.s) != hipSuccess) {
          set_error("local transport: hipMemcpyAsync failed", __FILE__, __LINE__);
          return FTAR_ERR_HIP;
        }
    }
    return FTAR_SUCCESS;
  }

  // hand every message taken so far back to its sender: with its stream's copies-done event (one per
  // receiving stream), or none if this rank failed (the sender then fails too, at once, instead of waiting
  // out the timeout)
  ftar_status_t hand_back(Flush& f, ftar_status_t st) {
    if (st != FTAR_SUCCESS) {
      // a failed flush hands the senders their messages back only once the copies it already enqueued from
      // them have finished, so a failed sender that returns at once may free or reuse its buffer;
      // the receiving streams wait only on the senders' data-ready events, recorded before the senders wait
      // for anything of this flush, so these synchronisations end
      std::vector<hipStream_t> seen;
      for (auto& x : f.got)
        if (std::find(seen.begin(), seen.end(), x.second) == seen.end()) {
          seen.push_back(x.second);
          hip_ignore(hipStreamSynchronize(x.second));
        }
    }
    for (auto& x : f.got) {
      Ev* e = slot_for(f.done, x.second);
      if (st != FTAR_SUCCESS || *e) continue;
      st = hub_->take_shared(e);
      if (st == FTAR_SUCCESS && hipEventRecord(**e, x.second) != hipSuccess) {
        set_error("local transport: hipEventRecord failed", __FILE__, __LINE__);
        st = FTAR_ERR_HIP;
      }
    }
    {
      std::lock_guard<std::mutex> g(hub_->mu);
      for (auto& x : f.got) {
        if (st == FTAR_SUCCESS) x.first->done = *slot_for(f.done, x.second);
        x.first->taken = true;
      }
    }
    for (auto& x : f.got) hub_->notify(x.first->sender);
    return st;
  }

  // 3. the sender's stream may not move on (and overwrite the source) before the copy
  ftar_status_t await_receivers(const std::vector<Op>& ops, Flush& f) {
    f.waited.clear();
    size_t i = 0;
    for (auto& o : ops) {
      if (!o.is_send) continue;
      auto& p = f.mine[i++];
      Ev d;
      {
        std::unique_lock<std::mutex> g(hub_->mu);
        if (!hub_->wait(g, rank_, [&] { return p->taken || !hub_->broken.empty(); })) {
          set_error("local transport: send to rank " + std::to_string(o.peer) + " never received", __FILE__,
                    __LINE__);
          return FTAR_ERR_TIMEOUT;
        }
        if (!p->taken) {
          set_error("local transport: another rank failed before receiving (" + hub_->broken + ")", __FILE__,
                    __LINE__);
          return FTAR_ERR_INTERNAL;
        }
        d = p->done;
      }
      if (!d) {
        set_error("local transport: rank " + std::to_string(o.peer) + " failed to receive", __FILE__, __LINE__);
        return FTAR_ERR_INTERNAL;
      }
      const std::pair<hipStream_t, hipEvent_t> w{o.s, *d};
      if (std::find(f.waited.begin(), f.waited.end(), w) == f.waited.end()) {
        FTAR_CHECK_HIP(hipStreamWaitEvent(o.s, *d, 0));
        f.waited.push_back(w);
      }
    }
    return FTAR_SUCCESS;
  }

  std::shared_ptr<LocalHub> hub_;
  int rank_;
  int depth_ = 0;
  std::vector<Op> ops_;
};

}  // namespace

std::unique_ptr<Transport> make_local_transport(std::shared_ptr<LocalHub> hub, int rank) {
  return std::unique_ptr<Transport>(new LocalTransport(std::move(hub), rank));
}

}  // namespace ftar
