// kg_comm.hpp -- the communicator as the units that speak through it see it: kg_comm.hip (the transports, liveness, the small
// collectives), kg_comm_exchange.hip (the exchange protocol), and the gathered paths, kg_jf_device.hip, kg_query.hip and kg_per_record.hip.
// What a gathered call's ranks settle among themselves is here once: that they were given the same call (comm_agree_on_call), that all
// of them can start (comm_agree_to_start, with gathered_peer_error's words for a peer that cannot) and how it ended (comm_agree_done).
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

// comm_agree_to_start's peer_error of a gathered call, into c: "<name>: rank p of w has no device memory for <room>", room_fmt being the
// call's words for what a rank found no room for, with one %zu (room) -- "a batch of %zu bases" --, or "<name>: rank p could not read its table".
std::function<int(int who, int code)> gathered_peer_error(katgpu_comm* m, katgpu_ctx* c, const char* name, const char* room_fmt, size_t room);

// ---- the same call on every rank (kg_comm.hip) ----
// A gathered call cuts its batches from its arguments, and a rank that cut them differently would wait in a collective of a batch that its
// peers do not have, until the liveness timeout.  So, before anything else, one allgather_u64 of every rank's
//   n | k | n_rec | a checksum of the records' starts and lengths | "my arguments are unusable" | the call's extra words
// and the same verdict on every rank: KATGPU_OK, or KATGPU_ERR_INVALID_ARG with the text in c, `name` in front, for the first of
//   1. a rank whose arguments are unusable (the lowest such rank; unusable_what says of what: "was given no bases, or rank 0 no room for ...");
//   then, rank by rank against rank 0:
//   2. another n, n_rec or k;  3. records that are not where rank 0's are;  4. other extra words (extra->differ: "count ranges are not rank 0's").
// recs: the records of a per-record call, null for a call that has none.  Their checksum is taken only where the arguments are usable.
struct CallRecords { const uint64_t *start, *len; size_t n; };
struct CallWords { const uint64_t* words; size_t n; const char* differ; };
int comm_agree_on_call(katgpu_comm* m, katgpu_ctx* c, const char* name, size_t n, uint32_t k, const CallRecords* recs, bool unusable, const char* unusable_what,
                       const CallWords* extra = nullptr);

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
