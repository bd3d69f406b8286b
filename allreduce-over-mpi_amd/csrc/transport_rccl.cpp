// The RCCL transport: one process per GPU, ncclSend/ncclRecv inside ncclGroupStart/End over xGMI (the
// product path).
//
// The reference moves every block with MPI_Isend/MPI_Irecv, tag 0, matched in
// posting order per peer pair, and then blocks in MPI_Waitall + MPI_Barrier
// (mpi_mod.hpp:1254-1305, :1576-1595, :1696-1712).  Here a stage's moves are
// one group of non-blocking, stream-ordered p2p operations; completion is a
// stream event, never a host wait or a barrier.
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cstring>

#include "transport_ipc.h"

namespace ftar {
namespace {

// ncclGetLastError(NULL) adds RCCL's own detail of the failure (which peer, which transport) to the
// status string: one driver record of a failed first RCCL contact then says why (bench.py gathers every
// rank's ftar_last_error)
std::string nccl_error_text(const char* expr, ncclResult_t r) {
  const char* d = ncclGetLastError(nullptr);
  return std::string(expr) + ": " + ncclGetErrorString(r) + (d && *d ? std::string(" (") + d + ")" : std::string());
}

#define FTAR_CHECK_NCCL(expr)                                              \
  do {                                                                     \
    ncclResult_t _r = (expr);                                              \
    if (_r != ncclSuccess) {                                               \
      ::ftar::set_error(nccl_error_text(#expr, _r), __FILE__, __LINE__);   \
      return FTAR_ERR_RCCL;                                                \
    }                                                                      \
  } while (0)

class RcclTransport final : public Transport {
 public:
  explicit RcclTransport(ncclComm_t c) : comm_(c) {
    if (ncclCommCount(comm_, &nranks_) != ncclSuccess || nranks_ < 1) nranks_ = 1;
    // the agreement's buffer and stream exist before any agreement is attempted, so a rank never leaves
    // its peers waiting in that collective because an allocation failed at its start
    if (hipMalloc(&agree_buf_, kAgreeBytes * (size_t)(nranks_ + 1) + 2 * (size_t)nranks_) != hipSuccess ||
        hipStreamCreateWithFlags(&agree_s_, hipStreamNonBlocking) != hipSuccess) {
      (void)hipGetLastError();
      agree_ready_ = false;
    }
  }
  ~RcclTransport() override {
    if (comm_ && !aborted_.load()) ncclCommDestroy(comm_);
    if (agree_s_) hip_ignore(hipStreamDestroy(agree_s_));
    if (agree_buf_) hip_ignore(hipFree(agree_buf_));
    if (scratch_) hip_ignore(hipFree(scratch_));
  }
  bool first_contact_blocks() const override { return true; }
  // one byte each way with every peer in one group, waited for: RCCL connects a p2p pair lazily, inside the
  // ncclGroupEnd of its first ncclSend/ncclRecv, and that connection handshake blocks the host until the peer
  // makes the same call (tools/rccl_order: two communicators whose first exchanges were issued in opposite
  // orders hung there); done once at a communicator's first contact, no later call blocks on it
  ftar_status_t connect_peers(int rank) override {
    if (nranks_ < 2) return FTAR_SUCCESS;
    if (!agree_ready_) {
      set_error("RCCL transport: no agreement buffer (allocation at bring-up failed)", __FILE__, __LINE__);
      return FTAR_ERR_NO_MEMORY;
    }
    char* base = static_cast<char*>(agree_buf_) + kAgreeBytes * (size_t)(nranks_ + 1);
    bool ok = ncclGroupStart() == ncclSuccess;
    for (int q = 0; q < nranks_ && ok; ++q)
      if (q != rank)
        ok = ncclSend(base + q, 1, ncclUint8, q, comm_, agree_s_) == ncclSuccess &&
             ncclRecv(base + nranks_ + q, 1, ncclUint8, q, comm_, agree_s_) == ncclSuccess;
    ok = ncclGroupEnd() == ncclSuccess && ok;
    ok = ok && hipStreamSynchronize(agree_s_) == hipSuccess;
    if (!ok) {
      set_error("RCCL transport: connecting the peers (one byte each way) failed", __FILE__, __LINE__);
      return FTAR_ERR_RCCL;
    }
    return FTAR_SUCCESS;
  }
  // comm_ itself is never cleared: the first-contact helper thread may still be reading it inside an RCCL
  // call, which the abort makes return; the destructor, which runs after that helper has
  // finished, then skips ncclCommDestroy
  void abort() override {
    if (comm_ && !aborted_.exchange(true)) ncclCommAbort(comm_);
  }
  // a 4-byte all-reduce: complete on any rank's stream only once every rank's
  // stream has reached it
  ftar_status_t barrier(hipStream_t s) override {
    FTAR_RETURN_IF(ensure_scratch());
    FTAR_CHECK_NCCL(ncclAllReduce(scratch_, scratch_, 1, ncclInt32, ncclSum, comm_, s));
    return FTAR_SUCCESS;
  }
  // IPC references (allocation handle + offset) of every rank's pointer,
  // all-gathered over RCCL, opened here (dmabuf IPC; peer access enabled
  // lazily by the runtime)
  ftar_status_t map_peers(void* mine, int rank, int nranks, std::vector<char*>* peers) override {
    if (nranks != nranks_ || rank < 0 || rank >= nranks) return FTAR_ERR_INVALID_ARG;
    FTAR_RETURN_IF(ensure_scratch());
    IpcRef ref;
    std::string why;
    if (ipc_export(mine, &ref) != FTAR_SUCCESS) why = std::string("rank ") + std::to_string(rank) + ": " + last_error();
    std::vector<IpcRef> all(nranks);
    char* dev = static_cast<char*>(scratch_) + 256;  // nranks refs after the barrier and agreement words
    FTAR_RETURN_IF(on_private_stream("peer map: handle exchange failed", [&](hipStream_t s) {
      return hipMemcpyAsync(dev + (size_t)rank * sizeof ref, &ref, sizeof ref, hipMemcpyHostToDevice, s) == hipSuccess &&
             ncclAllGather(dev + (size_t)rank * sizeof ref, dev, sizeof ref, ncclUint8, comm_, s) == ncclSuccess &&
             hipMemcpyAsync(all.data(), dev, (size_t)nranks * sizeof ref, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipStreamSynchronize(s) == hipSuccess;
    }));
    int failed = 0;
    FTAR_RETURN_IF(open_peers_in_turns(
        all, mine, rank, imports_, [this](int mine_failed, int* total) { return agree_failures(mine_failed, total); },
        peers, &failed, &why));
    if (failed) {
      set_error(why.empty() ? std::to_string(failed) + " peer rank(s) could not map the exchange buffers" : why,
                __FILE__, __LINE__);
      return FTAR_ERR_HIP;
    }
    return FTAR_SUCCESS;
  }
  void unmap_peers(std::vector<char*>* peers, int rank) override { imports_.close_all(peers, rank); }
  ftar_status_t group_start() override {
    FTAR_CHECK_NCCL(ncclGroupStart());
    return FTAR_SUCCESS;
  }
  ftar_status_t send(const void* buf, size_t bytes, int peer, hipStream_t s) override {
    FTAR_CHECK_NCCL(ncclSend(buf, bytes, ncclUint8, peer, comm_, s));
    return FTAR_SUCCESS;
  }
  ftar_status_t recv(void* buf, size_t bytes, int peer, hipStream_t s) override {
    FTAR_CHECK_NCCL(ncclRecv(buf, bytes, ncclUint8, peer, comm_, s));
    return FTAR_SUCCESS;
  }
  ftar_status_t group_end() override {
    FTAR_CHECK_NCCL(ncclGroupEnd());
    return FTAR_SUCCESS;
  }
  const char* name() const override { return "rccl"; }
  bool uses_ipc() const override { return true; }
  bool masked_reduce_stream_ok() const override { return false; }
  ftar_status_t allgather(const void* send, void* recv, size_t bytes, int rank, int nranks, hipStream_t s) override {
    (void)rank;
    (void)nranks;
    FTAR_CHECK_NCCL(ncclAllGather(send, recv, bytes, ncclUint8, comm_, s));
    return FTAR_SUCCESS;
  }
  ftar_status_t native_allreduce(const void* send, void* recv, size_t count, ftar_dtype_t dt, ftar_op_t op,
                                 hipStream_t s) override {
    ncclDataType_t t;
    switch (dt) {
      case FTAR_UINT8: t = ncclUint8; break;
      case FTAR_INT8: t = ncclInt8; break;
      case FTAR_INT32: t = ncclInt32; break;
      case FTAR_INT64: t = ncclInt64; break;
      case FTAR_FLOAT32: t = ncclFloat32; break;
      case FTAR_FLOAT64: t = ncclFloat64; break;
      case FTAR_BFLOAT16: t = ncclBfloat16; break;
      case FTAR_FLOAT16: t = ncclFloat16; break;
#if defined(RCCL_FLOAT8) && RCCL_FLOAT8  // RCCL's own fp8 conversion: it may saturate where ftar's overflows
      case FTAR_FLOAT8_E4M3: t = ncclFloat8e4m3; break;
      case FTAR_FLOAT8_E5M2: t = ncclFloat8e5m2; break;
#endif
      default: return FTAR_ERR_UNSUPPORTED;
    }
    ncclRedOp_t o;
    switch (op) {  // RCCL's own arithmetic: its NaN and signed-zero rules for max / min are not ftar's contract
      case FTAR_SUM: o = ncclSum; break;
      case FTAR_MAX: o = ncclMax; break;
      case FTAR_MIN: o = ncclMin; break;
      case FTAR_AVG:  // RCCL's mean: integers too, by its own rules; ftar's AVG is the float dtypes'
        if (!dtype_scalable(dt)) return FTAR_ERR_UNSUPPORTED;
        o = ncclAvg;
        break;
      default: return FTAR_ERR_UNSUPPORTED;
    }
    FTAR_CHECK_NCCL(ncclAllReduce(send ? send : recv, recv, count, t, o, comm_, s));
    return FTAR_SUCCESS;
  }

  void* rccl_register(void* buf, size_t bytes) override {
    void* h = nullptr;
    if (ncclCommRegister(comm_, buf, bytes, &h) != ncclSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    return h;
  }
  void rccl_deregister(void* handle) override {
    if (handle && !aborted_.load()) (void)ncclCommDeregister(comm_, handle);
  }
  // every rank's bytes through one ncclAllGather on a private stream (host-blocking; communicator
  // bring-up only)
  ftar_status_t agree(const void* mine, size_t bytes, bool* same) override {
    if (bytes > kAgreeBytes || !agree_ready_) {
      set_error("settings agreement: no agreement buffer, or more than 256 bytes to agree on", __FILE__, __LINE__);
      return FTAR_ERR_INTERNAL;
    }
    char* dev = static_cast<char*>(agree_buf_);
    std::vector<char> all((size_t)nranks_ * bytes);
    const bool ok = hipMemcpyAsync(dev, mine, bytes, hipMemcpyHostToDevice, agree_s_) == hipSuccess &&
                    ncclAllGather(dev, dev + kAgreeBytes, bytes, ncclUint8, comm_, agree_s_) == ncclSuccess &&
                    hipMemcpyAsync(all.data(), dev + kAgreeBytes, all.size(), hipMemcpyDeviceToHost, agree_s_) ==
                        hipSuccess &&
                    hipStreamSynchronize(agree_s_) == hipSuccess;
    if (!ok) {
      set_error("settings agreement: the all-gather failed", __FILE__, __LINE__);
      return FTAR_ERR_RCCL;
    }
    *same = all_same(all.data(), mine, bytes, nranks_);
    return FTAR_SUCCESS;
  }

 private:
  static constexpr size_t kAgreeBytes = 256;
  void* agree_buf_ = nullptr;  // one agreement per rank (all-gathered) + the connection bytes
  hipStream_t agree_s_ = nullptr;
  bool agree_ready_ = true;

  // a host-blocking exchange on a non-blocking stream of its own, made for it and destroyed after it:
  // issue(s) enqueues the exchange on s and waits for s; false: it failed, reported as `what`
  template <class F>
  ftar_status_t on_private_stream(const char* what, F&& issue) {
    hipStream_t s;
    FTAR_CHECK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    const bool ok = issue(s);
    hip_ignore(hipStreamDestroy(s));
    if (!ok) {
      set_error(what, __FILE__, __LINE__);
      return FTAR_ERR_RCCL;
    }
    return FTAR_SUCCESS;
  }
  // sum of every rank's `mine` (host-blocking, on a private stream)
  ftar_status_t agree_failures(int mine, int* total) {
    int* word = reinterpret_cast<int*>(static_cast<char*>(scratch_) + 128);
    return on_private_stream("peer map: failure agreement failed", [&](hipStream_t s) {
      return hipMemcpyAsync(word, &mine, sizeof mine, hipMemcpyHostToDevice, s) == hipSuccess &&
             ncclAllReduce(word, word, 1, ncclInt32, ncclSum, comm_, s) == ncclSuccess &&
             hipMemcpyAsync(total, word, sizeof *total, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipStreamSynchronize(s) == hipSuccess;
    });
  }
  // barrier word, agreement word, one IPC reference per rank (map_peers all-gathers nranks of them)
  ftar_status_t ensure_scratch() {
    if (!scratch_) FTAR_CHECK_HIP(hipMalloc(&scratch_, 256 + (size_t)std::max(nranks_, 1) * sizeof(IpcRef)));
    return FTAR_SUCCESS;
  }
  ncclComm_t comm_;
  std::atomic<bool> aborted_{false};
  int nranks_ = 1;
  void* scratch_ = nullptr;
  PeerImports imports_;
};

}  // namespace

std::unique_ptr<Transport> make_rccl_transport(int nranks, const ftar_unique_id_t& id, int rank, ftar_status_t* st) {
  static_assert(sizeof(ftar_unique_id_t) == sizeof(ncclUniqueId), "unique id size");
  ncclUniqueId uid;
  memcpy(&uid, &id, sizeof(uid));
  ncclComm_t c = nullptr;
  ncclResult_t r = ncclCommInitRank(&c, nranks, uid, rank);
  if (r != ncclSuccess) {
    set_error(nccl_error_text("ncclCommInitRank", r), __FILE__, __LINE__);
    *st = FTAR_ERR_RCCL;
    return nullptr;
  }
  *st = FTAR_SUCCESS;
  return std::unique_ptr<Transport>(new RcclTransport(c));
}

}  // namespace ftar
