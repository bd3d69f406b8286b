// IPC plumbing of the peer-direct forms: exportable allocations, references to them (export, import with
// a verified mapping, the tokens that verify it), the per-process table of imported peer allocations, and
// the turn-taking protocol by which the ranks of the RCCL and the host-bootstrapped transports map each
// other's buffers (transport_ipc.h).
#include <unistd.h>

#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <random>

#include "transport_ipc.h"

namespace ftar {

bool ipc_size_guard() {
  static const bool on = [] {
    if (const char* e = getenv("FTAR_IPC_SIZE_GUARD")) return *e != '0';
    int v = 0;
    return hipRuntimeGetVersion(&v) != hipSuccess || v < 70200000;  // major*1e7 + minor*1e5 + patch
  }();
  return on;
}

// Exportable sizes: at least 2 MiB, because the runtime sub-allocates small
// hipMalloc requests out of a shared block that hipMemGetAddressRange / IPC
// export do not see as an allocation of its own (a 4-byte exchange buffer for a
// one-element bucket failed "named symbol not found"); and round past sizes
// with bit 31 set where the runtime blocks opening them (guard: ipc_size_guard).
size_t ipc_safe_size_for(size_t bytes, bool guard) {
  const size_t bit31 = size_t(1) << 31, mask4g = (size_t(1) << 32) - 1, min_bytes = size_t(2) << 20;
  bytes = std::max(bytes, min_bytes);
  return (guard && (bytes & bit31)) ? (bytes | mask4g) + 1 : bytes;  // up to the next 4 GiB
}

size_t ipc_safe_size(size_t bytes) { return ipc_safe_size_for(bytes, ipc_size_guard()); }

namespace {
std::mutex g_tokens_mu;
std::map<const void*, std::array<uint64_t, 2>> g_tokens;  // stamped buffers (owned exchange/bounce buffers)
}

void forget_token(const void* p) {
  std::lock_guard<std::mutex> g(g_tokens_mu);
  g_tokens.erase(p);
}

ftar_status_t alloc_exportable(size_t bytes, bool ipc, void** out, size_t* got) {
  const size_t want = ipc ? ipc_safe_size(bytes) : bytes;
  *out = nullptr;
  *got = 0;
  std::vector<void*> set_aside;
  ftar_status_t st = FTAR_ERR_HIP;
  for (int attempt = 0; attempt < 4; ++attempt) {
    void* fresh = nullptr;
    const hipError_t me = hipMalloc(&fresh, want);
    if (me != hipSuccess) {
      (void)hipGetLastError();
      set_error("hipMalloc of " + std::to_string(want) + " bytes failed", __FILE__, __LINE__);
      if (me == hipErrorOutOfMemory) st = FTAR_ERR_NO_MEMORY;
      break;
    }
    IpcRef probe;
    if (!ipc || ipc_export(fresh, &probe) == FTAR_SUCCESS) {
      *out = fresh;
      *got = want;
      st = FTAR_SUCCESS;
      break;
    }
    trace("%p not exportable, allocating another", fresh);
    set_aside.push_back(fresh);
  }
  for (void* p : set_aside) hip_ignore(hipFree(p));
  return st;
}

ftar_status_t ipc_export(const void* p, IpcRef* out) {
  memset(out, 0, sizeof *out);
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  FTAR_CHECK_HIP(hipMemGetAddressRange(&base, &size, const_cast<void*>(p)));
  trace("ipc_export %p: allocation %p + %zu bytes", p, (void*)base, size);
  if (ipc_size_guard() && (size & (size_t(1) << 31))) {
    set_error("IPC export of a " + std::to_string(size) +
                  "-byte allocation refused: this HIP runtime blocks in hipIpcOpenMemHandle for sizes with bit 31 "
                  "set (FTAR_IPC_SIZE_GUARD)",
              __FILE__, __LINE__);
    return FTAR_ERR_UNSUPPORTED;
  }
  out->offset = static_cast<uint64_t>(static_cast<const char*>(p) - static_cast<const char*>(base));
  const hipError_t e = hipIpcGetMemHandle(&out->handle, base);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // not sticky: the next launch check must not see it
    memset(&out->handle, 0, sizeof out->handle);
    set_error(std::string("hipIpcGetMemHandle: ") + hipGetErrorString(e), __FILE__, __LINE__);
    trace("ipc_export %p failed: %s", p, hipGetErrorString(e));
    return FTAR_ERR_HIP;
  }
  out->size = size;
  {
    std::lock_guard<std::mutex> g(g_tokens_mu);
    auto it = g_tokens.find(p);
    if (it != g_tokens.end()) {
      out->stamped = 1;
      out->token[0] = it->second[0];
      out->token[1] = it->second[1];
    }
  }
  if (!out->stamped && size - out->offset >= sizeof out->token) {
    // a caller's buffer (registration): its first 16 bytes as they are now -- the importers must read the
    // same through their mappings (the buffer may not be written while it is being registered)
    if (hipMemcpy(out->token, p, sizeof out->token, hipMemcpyDeviceToHost) == hipSuccess) out->stamped = 2;
    else (void)hipGetLastError();
  }
  out->valid = 1;
  return FTAR_SUCCESS;
}

ftar_status_t stamp_token(void* p) {
  std::array<uint64_t, 2> t;
  {
    std::lock_guard<std::mutex> g(g_tokens_mu);
    static std::mt19937_64 rng(std::random_device{}() ^ (uint64_t)getpid() << 32);
    t = {rng(), rng()};
  }
  FTAR_CHECK_HIP(hipMemcpy(p, t.data(), sizeof t, hipMemcpyHostToDevice));
  std::lock_guard<std::mutex> g(g_tokens_mu);
  g_tokens[p] = t;
  return FTAR_SUCCESS;
}

ftar_status_t ipc_import(const IpcRef& ref, void** base, char** p) {
  if (ref.valid != 1) {
    set_error("ipc_import: the peer's export failed", __FILE__, __LINE__);
    return FTAR_ERR_HIP;
  }
  trace("ipc_import: open (offset %llu)", (unsigned long long)ref.offset);
  FTAR_CHECK_HIP(hipIpcOpenMemHandle(base, ref.handle, hipIpcMemLazyEnablePeerAccess));
  *p = static_cast<char*>(*base) + ref.offset;
  // verify the mapping: the runtime has been seen to map the wrong memory after regrowth
  std::string bad;
  hipDeviceptr_t b2 = nullptr;
  size_t sz = 0;
  if (hipMemGetAddressRange(&b2, &sz, *p) == hipSuccess) {
    if (sz < ref.size) bad = "size " + std::to_string(sz) + " < " + std::to_string(ref.size);  // (rounding up is fine)
  } else {
    (void)hipGetLastError();
  }
  if (bad.empty() && ref.stamped) {
    uint64_t got[2] = {0, 0};
    if (hipMemcpy(got, *p, sizeof got, hipMemcpyDeviceToHost) != hipSuccess) {
      (void)hipGetLastError();  // cannot read it back here: keep the mapping unverified rather than lose it
      trace("ipc_import: mapping at %p not verifiable (token unreadable)", *base);
    } else if (got[0] != ref.token[0] || got[1] != ref.token[1]) {
      bad = "token mismatch";
    }
  }
  if (!bad.empty()) {
    trace("ipc_import: mapping at %p rejected (%s)", *base, bad.c_str());
    hip_ignore(hipIpcCloseMemHandle(*base));
    *base = nullptr;
    *p = nullptr;
    set_error("ipc_import: the mapping does not show the peer's buffer (" + bad + ")", __FILE__, __LINE__);
    return FTAR_ERR_HIP;
  }
  trace("ipc_import: mapped at %p (verified)", *base);
  return FTAR_SUCCESS;
}

ftar_status_t PeerImports::open(const IpcRef& ref, char** out) {
  const std::string key(reinterpret_cast<const char*>(&ref.handle), sizeof ref.handle);
  auto it = imports_.find(key);
  if (it == imports_.end()) {
    void* base = nullptr;
    char* p = nullptr;
    FTAR_RETURN_IF(ipc_import(ref, &base, &p));
    it = imports_.emplace(key, Import{base, 0}).first;
  }
  ++it->second.refs;
  *out = static_cast<char*>(it->second.base) + ref.offset;
  handed_.emplace(*out, key);
  return FTAR_SUCCESS;
}

void PeerImports::close(char* p) {
  auto h = handed_.find(p);
  if (h == handed_.end()) return;
  auto it = imports_.find(h->second);
  handed_.erase(h);
  if (it != imports_.end() && --it->second.refs == 0) {
    trace("ipc close %p", it->second.base);
    hip_ignore(hipIpcCloseMemHandle(it->second.base));
    imports_.erase(it);
  }
}

void PeerImports::close_all(std::vector<char*>* peers, int rank) {
  for (int q = 0; q < (int)peers->size(); ++q)
    if (q != rank && (*peers)[q]) close((*peers)[q]);
  peers->clear();
}

// The ranks open the peers' handles in turns (a precaution
// taken while chasing the 2 GiB open hang, ipc_size_guard, which turned
// out to be a runtime size bug; turns cost P host agreements per mapping,
// nothing per call).  Each turn ends with a host-side
// agreement on the failures so far, so every rank also learns whether
// every rank mapped every peer (a rank that failed alone would otherwise
// leave the others waiting in the next barrier).
ftar_status_t open_peers_in_turns(const std::vector<IpcRef>& all, void* mine, int rank, PeerImports& imports,
                                  const AgreeFailures& agree_failures, std::vector<char*>* peers, int* failed,
                                  std::string* why) {
  const int nranks = (int)all.size();
  peers->assign(nranks, nullptr);
  for (int q = 0; q < nranks && why->empty(); ++q)  // a failed export anywhere: nobody opens anything
    if (all[q].valid != 1) *why = std::string("rank ") + std::to_string(q) + " could not export its buffer";
  *failed = 0;
  for (int turn = 0; turn < nranks; ++turn) {
    if (turn == rank && why->empty() && !*failed) {
      for (int q = 0; q < nranks; ++q) {
        if (q == rank) {
          (*peers)[q] = static_cast<char*>(mine);
          continue;
        }
        if (imports.open(all[q], &(*peers)[q]) != FTAR_SUCCESS) {
          *why = std::string("rank ") + std::to_string(q) + ": " + last_error();
          break;
        }
      }
    }
    FTAR_RETURN_IF(agree_failures(why->empty() ? 0 : 1, failed));
  }
  if (*failed) imports.close_all(peers, rank);
  return FTAR_SUCCESS;
}

}  // namespace ftar
