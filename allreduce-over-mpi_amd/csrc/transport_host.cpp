// The host-bootstrapped transport: caller-bootstrapped processes (ftar_comm_init_host), peer-direct only.
//
// Point-to-point transfers are unsupported: the one-round plans run in the
// peer-direct forms (kernel loads/stores through IPC-mapped buffers), whose
// barriers and handle exchanges go through the caller's host allgather.
// (Round 1 carried an experimental host-synchronous bounce-buffer p2p here; a
// long 4-process run on one GPU stalled in it, and as no product path used it,
// it was removed.)
#include "transport_ipc.h"

namespace ftar {
namespace {
class HostTransport final : public Transport {
 public:
  HostTransport(int nranks, int rank, ftar_host_allgather_fn fn, void* user)
      : nranks_(nranks), rank_(rank), fn_(fn), user_(user) {}
  ftar_status_t group_start() override { return FTAR_SUCCESS; }
  ftar_status_t send(const void*, size_t, int, hipStream_t) override { return unsupported(); }
  ftar_status_t recv(void*, size_t, int, hipStream_t) override { return unsupported(); }
  ftar_status_t group_end() override { return FTAR_SUCCESS; }
  ftar_status_t allgather(const void*, void*, size_t, int, int, hipStream_t) override { return unsupported(); }
  const char* name() const override { return "host"; }
  bool uses_ipc() const override { return true; }
  bool async_p2p() const override { return false; }
  // everything before it on s, on every rank, is complete when it returns
  ftar_status_t barrier(hipStream_t s) override {
    bool ok = true;
    FTAR_RETURN_IF(barrier_status(s, true, &ok));
    if (!ok) {
      set_error("host transport: another rank failed before this barrier", __FILE__, __LINE__);
      return FTAR_ERR_INTERNAL;
    }
    return FTAR_SUCCESS;
  }
  // a failed stream synchronisation is this rank's failure, reported to the others rather than returned
  // before the host collective (which would leave them waiting in it)
  ftar_status_t barrier_status(hipStream_t s, bool mine_ok, bool* all_ok) override {
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      set_error(std::string("host transport barrier: hipStreamSynchronize: ") + hipGetErrorString(e), __FILE__,
                __LINE__);
      mine_ok = false;
    }
    const char mine = mine_ok ? 1 : 0;
    std::vector<char> all(nranks_);
    FTAR_RETURN_IF(gather(&mine, all.data(), 1));
    *all_ok = true;
    for (char v : all) *all_ok = *all_ok && v == 1;
    return FTAR_SUCCESS;
  }
  ftar_status_t agree(const void* mine, size_t bytes, bool* same) override {
    std::vector<char> all((size_t)nranks_ * bytes);
    FTAR_RETURN_IF(gather(mine, all.data(), bytes));
    *same = all_same(all.data(), mine, bytes, nranks_);
    return FTAR_SUCCESS;
  }
  // every rank's IPC reference through the caller's allgather, opened in turns whose failure agreement is
  // that allgather again (one flag per rank)
  ftar_status_t map_peers(void* mine, int rank, int nranks, std::vector<char*>* peers) override {
    if (nranks != nranks_ || rank != rank_) return FTAR_ERR_INVALID_ARG;
    IpcRef ref;
    (void)ipc_export(mine, &ref);  // a failed export is published like any other (valid = 0): every rank sees it
    std::vector<IpcRef> all(nranks);
    FTAR_RETURN_IF(gather(&ref, all.data(), sizeof ref));
    std::vector<int> flags(nranks);
    int failed = 0;
    std::string why;
    FTAR_RETURN_IF(open_peers_in_turns(
        all, mine, rank, imports_,
        [&](int mine_failed, int* total) -> ftar_status_t {
          FTAR_RETURN_IF(gather(&mine_failed, flags.data(), sizeof mine_failed));
          *total = 0;
          for (int f : flags) *total += f;
          return FTAR_SUCCESS;
        },
        peers, &failed, &why));
    if (failed) {
      set_error("host transport: a rank could not map the peers' buffers", __FILE__, __LINE__);
      return FTAR_ERR_HIP;
    }
    return FTAR_SUCCESS;
  }
  void unmap_peers(std::vector<char*>* peers, int rank) override { imports_.close_all(peers, rank); }

 private:
  static ftar_status_t unsupported() {
    set_error("host transport: point-to-point transfers are unsupported (one-round plans in the peer-direct "
              "forms only)",
              __FILE__, __LINE__);
    return FTAR_ERR_UNSUPPORTED;
  }
  ftar_status_t gather(const void* mine, void* all, size_t bytes) {
    if (fn_(mine, all, bytes, user_) != 0) {
      set_error("host transport: the caller's allgather failed", __FILE__, __LINE__);
      return FTAR_ERR_INTERNAL;
    }
    return FTAR_SUCCESS;
  }
  int nranks_, rank_;
  ftar_host_allgather_fn fn_;
  void* user_;
  PeerImports imports_;
};
}  // namespace

std::unique_ptr<Transport> make_host_transport(int nranks, int rank, ftar_host_allgather_fn fn, void* user) {
  return std::unique_ptr<Transport>(new HostTransport(nranks, rank, fn, user));
}

}  // namespace ftar
