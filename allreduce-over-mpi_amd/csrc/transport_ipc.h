// What the two IPC transports (transport_rccl.cpp, transport_host.cpp) share; defined in ipc.cpp.
#pragma once

#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "ftar_internal.h"

namespace ftar {
#pragma GCC visibility push(hidden)  // private to those three translation units: not in the library's symbol table

// Peer allocations imported into this process: one IPC mapping per allocation
// (two registered buffers may share one), reference-counted by the pointers
// handed out, so closing one pointer never unmaps memory another still uses.
class PeerImports {
 public:
  ftar_status_t open(const IpcRef& ref, char** out);
  void close(char* p);
  // every peer pointer of a map_peers result (the own slot is not an import)
  void close_all(std::vector<char*>* peers, int rank);

 private:
  struct Import {
    void* base;
    int refs;
  };
  std::map<std::string, Import> imports_;     // peer allocation (IPC handle bytes) -> its mapping here
  std::multimap<char*, std::string> handed_;  // peer pointer handed out -> its allocation
};

// The collective half of map_peers after the transport has gathered every rank's reference into `all`:
// *peers = every rank's pointer as mapped here (peers[rank] = mine), all ranks or none.
//   - a failed export anywhere (a reference with valid != 1): nobody opens anything;
//   - the ranks open in turns, rank `turn` in turn `turn`, and every turn ends with agree_failures(this
//     rank has failed so far, the number of ranks that have): the transport's host-blocking collective;
//   - once a failure is agreed on, the later turns open nothing (they still agree: every rank runs the
//     same number of collectives);
//   - *failed = the ranks that had failed after the last turn; when there are any, everything opened here
//     is closed again and *peers is empty.  *why = this rank's own failure, if it had one (the caller may
//     pass its failed export's reason in it).
// Returns what agree_failures returned when that failed (nothing is unmapped then: the transport is
// broken), else FTAR_SUCCESS: the caller reports *failed in its own words.
using AgreeFailures = std::function<ftar_status_t(int mine_failed, int* total)>;
ftar_status_t open_peers_in_turns(const std::vector<IpcRef>& all, void* mine, int rank, PeerImports& imports,
                                  const AgreeFailures& agree_failures, std::vector<char*>* peers, int* failed,
                                  std::string* why);

// Transport::agree's verdict: every rank's `bytes` (all: nranks of them, in rank order) equal mine
inline bool all_same(const void* all, const void* mine, size_t bytes, int nranks) {
  bool same = true;
  for (int q = 0; q < nranks; ++q) same = same && !memcmp(static_cast<const char*>(all) + (size_t)q * bytes, mine, bytes);
  return same;
}

#pragma GCC visibility pop
}  // namespace ftar
