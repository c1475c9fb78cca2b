// kg_comm.hpp -- the communicator as the units that speak through it see it: kg_comm.hip (the transports, liveness, the small
// collectives), kg_comm_exchange.hip (the exchange protocol), and the gathered paths, kg_jf_device.hip and kg_query.hip.
// Nobody else includes it: the rest of the library and its callers know katgpu_comm as the opaque handle of include/katgpu.h.
#pragma once
#include "kg_host.hpp"

typedef struct ncclComm* ncclComm_t;          // (as <rccl/rccl.h> has it: only kg_comm.hip includes that)
struct ShmHeader; struct RankBeat;            // the rendezvous block in /dev/shm (kg_comm.hip)
struct Exchange;                              // kg_comm_exchange.hip

struct katgpu_comm {
    katgpu_ctx* ctx = nullptr;
    int rank = 0, world = 1;
    bool use_rccl = false;
    ncclComm_t nccl = nullptr;
    hipStream_t stream = nullptr;             // transport stream: chunk c travels while chunk c-1 is merged on the context's stream
    hipEvent_t ev[2] = {nullptr, nullptr};
    std::string token;
    ShmHeader* hdr = nullptr; RankBeat* beats = nullptr; uint8_t* boxes = nullptr; size_t shm_bytes = 0;
    std::thread beat_thread; std::atomic<bool> beat_stop{false};
    int distinct_devices = 1;                 // how many different devices the ranks run on (1: they all share one)
    uint64_t seq = 0;                         // names the shm files of successive transfers
    double ms_exchange = 0, ms_merge = 0, ms_extract = 0, ms_allreduce = 0;
    uint64_t bytes_sent = 0, merge_launches = 0;
    uint64_t records_sent = 0, record_bytes_sent = 0;          // what katgpu_exchange_merge put on the wire as records (not the count matrices, not the all-reduce)
    std::vector<Exchange*> pending;                            // Exchanges begun (katgpu_exchange_begin) and not yet finished, oldest first (at most two)
    bool wire_packed = false;                                  // the last exchange's records: 9 bytes (remainder + count) or 12 (key + count)
    std::string transport_note;
    uint8_t* host_stage = nullptr; size_t host_stage_bytes = 0;
};
void drop_pending(katgpu_comm* m);            // an exchange begun and never finished: its buffers go with the communicator (kg_comm_exchange.hip)

// ---- the transport (kg_comm.hip).  Every rank of the communicator calls these together; a wait ends with an error, not a hang,
// when a peer has failed or died (liveness) ----
struct CommMsg { int peer; void* dev; size_t bytes; };          // one side of a point-to-point transfer (device memory)
// the error text into the context, and the abort flag raised: the peers are, or will be, waiting for this rank
int comm_fail(katgpu_comm* m, int code, const char* fmt, ...);
// this rank gives up inside a collective: its peers leave their waits with an error instead of waiting for it
void comm_abort(katgpu_comm* m);
int shm_barrier(katgpu_comm* m);
// the transport stream, or an event on it, waited for under the liveness checks
int comm_wait(katgpu_comm* m, hipEvent_t ev /* or null: the whole stream */, const char* what);
// A group of point-to-point transfers.  RCCL: asynchronous on m->stream, ev is recorded behind it and transfer_wait(ev) waits for it.
// SHM: done when transfer returns.  A message of no bytes is not sent; the n-th message to a peer meets the n-th from it.
int transfer(katgpu_comm* m, const std::vector<CommMsg>& sends, const std::vector<CommMsg>& recvs, hipEvent_t ev);
int transfer_wait(katgpu_comm* m, hipEvent_t ev);
inline int transfer_sync(katgpu_comm* m, const std::vector<CommMsg>& sends, const std::vector<CommMsg>& recvs) {      // ... done when it returns, on either transport
    const int rc = transfer(m, sends, recvs, m->ev[0]);
    return rc ? rc : transfer_wait(m, m->ev[0]);
}
// out[r * n ..) = rank r's n words (host arrays)
int allgather_u64(katgpu_comm* m, const uint64_t* mine, size_t n, uint64_t* out);

// ---- all go on, or none does (kg_comm.hip) ----
// Every rank says a word (one allgather_u64 of one word): *who = the first rank whose word is not 0, or -1, and *what = that word.
int comm_agree(katgpu_comm* m, uint64_t mine, int* who, uint64_t* what = nullptr);
// The two moments of a gathered path, rc being what this rank has met so far.  What went wrong on a rank is kept until everyone has
// heard of it: a rank that left early would leave its peers in a collective.
// Before the work, when everything a rank can need has been allocated or read: 0 when every rank can go on.  The rank that cannot
// returns its rc, its own error text in place; its peers get peer_error(who, code) -- the caller's words into the context, code
// returned -- with KATGPU_ERR_NOMEM when that rank had no memory and KATGPU_ERR_DEVICE for anything else.
int comm_agree_to_start(katgpu_comm* m, int rc, const std::function<int(int who, int code)>& peer_error);
// After the work: a rank that failed raises the abort flag (its peers' waits end), keeps its error text and returns its rc --
// KATGPU_ERR_DEVICE for KATGPU_ERR_NOMEM, which is the collective one of the moment before; its peers get the communicator's failure,
// or KATGPU_ERR_DEVICE with rank_failed_fmt (one %d: the rank).
int comm_agree_done(katgpu_comm* m, int rc, const char* rank_failed_fmt);

// what the ranks of a gathered per-record call compare of their records: every start and length, in order, folded into one word
inline uint64_t records_checksum(const uint64_t* rec_start, const uint64_t* rec_len, size_t n_rec) {
    uint64_t h = 0x9E3779B97F4A7C15ULL;
    auto fold = [&](uint64_t x) { h ^= x; h *= 0xFF51AFD7ED558CCDULL; h ^= h >> 32; };
    for (size_t r = 0; r < n_rec; ++r) { fold(rec_start[r]); fold(rec_len[r]); }
    return h;
}

// ---- the gather of a profile from the ranks' tables (kg_query.hip), for the collectives built on it: katgpu_table_profile_gathered_host
// there, katgpu_table_record_stats_gathered_host in kg_per_record.hip.  One object per collective call; its counters add up over gather(). ----
struct ProfileGather {
    katgpu_comm* comm; katgpu_table* t; int canonicalise;
    size_t batch = 0;                             // window starts per batch (KATGPU_TEST_GATHER_BATCH)
    size_t idx_off = 0, len_off = 0;
    DevBuf db, run, dense;                        // a batch's bases (stage_bases) | its run: counts, indices, length | its dense counts on rank 0 (stage_counts)
    uint64_t n_batches = 0, records = 0, wire_bytes = 0;
    // Before the work (comm_agree_to_start): the table read, the buffers of a batch of at most max_starts window starts from the pool.
    // stage_bases: gather() will be given host bases; stage_counts: it will send the counts to the host.
    int prepare(size_t max_starts, bool stage_bases, bool stage_counts);
    // Every rank, with the same n bases (n < k: nothing happens): from the host (bases) or already on this rank's device (dev_bases, which
    // wins).  On rank 0 the n - k + 1 counts go to the host array `counts`, or stay in the device array dev_counts (which wins).
    int gather(const char* bases, const uint8_t* dev_bases, size_t n, uint64_t* counts, uint64_t* dev_counts);
    void print_timing() const;                    // rank 0, under KATGPU_TIMING: the "profile_gathered" line of the call
};
int gather_peer_error(katgpu_comm* comm, const ProfileGather& g, int p, int code);      // comm_agree_to_start's peer_error for prepare()
