// kg_comm.hip -- the communicator behind the C ABI: katgpu_comm_* / katgpu_allreduce_u64, and what the units above it are given
// (kg_comm.hpp): the transports, liveness, the small collectives and the all-or-none agreements.  What travels through it and why:
// kg_comm_exchange.hip (the exchange of the ranks' tables), kg_jf_device.hip and kg_query.hip (the gathered .jf dump and profile).
//
// Transports.  RCCL (dlopen'ed: a single-GPU process never loads it): one ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd per
// chunk on a stream of its own -- every peer at once, which is the shape xGMI's point-to-point links want -- and ncclAllGather /
// ncclAllReduce for the small things.  SHM: ranks of one node stage their records through files in /dev/shm; slow, exact, needs
// nothing but a shared file system -- it is what carries ranks that SHARE a GPU (the test suite on a one-GPU box: RCCL refuses two
// ranks on one device).  Ranks on DISTINCT devices never take it by accident: a communicator that cannot have RCCL there fails
// (katgpu_comm_init says why) unless the caller asked for the staging transport by name (KATGPU_COMM_TRANSPORT=shm) or allowed the
// fall-back (KATGPU_COMM_ALLOW_SHM=1) -- a /dev/shm number must not pass for an xGMI one.  KATGPU_COMM_TRANSPORT = rccl | shm | auto.
// The protocols above the transport are the same code.
//
// Liveness.  Ranks may reach a collective minutes apart (`kat --gpus N` deals whole .gz files rank by rank), so no wait is bounded by
// a wall clock: every rank's communicator runs a heartbeat (a counter in the shared block, advanced every 50 ms by a thread of its
// own), and a wait gives up only when a peer has raised the abort flag or when a peer's heartbeat has stood still for
// KATGPU_COMM_TIMEOUT_S (default 60 s): a peer that died, not one that is busy.  KATGPU_COMM_MAX_WAIT_S (default: none) bounds a
// single wait by the clock for harnesses that prefer an error to a wedged link (bench.py sets it).
#include "kg_comm.hpp"

#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

namespace {

// ---- RCCL through dlopen ----
struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};
Rccl& rccl() {
    static Rccl r;
    static bool tried = false;
    if (tried) return r;
    tried = true;
    // (tests: KATGPU_RCCL_LIB names a stand-in that lets ranks SHARING a GPU take this branch -- tests/native/fake_rccl.cc; read only
    // under KATGPU_TESTING=1, like every hook)
    if (const char* test_lib = hook("KATGPU_RCCL_LIB")) r.lib = dlopen(test_lib, RTLD_NOW | RTLD_LOCAL);
    else
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            r.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (r.lib) break;
        }
    if (!r.lib) return r;
#define KG_SYM(F) r.F = reinterpret_cast<decltype(r.F)>(dlsym(r.lib, "nccl" #F))
    KG_SYM(GetUniqueId); KG_SYM(CommInitRank); KG_SYM(CommDestroy); KG_SYM(GroupStart); KG_SYM(GroupEnd); KG_SYM(Send); KG_SYM(Recv);
    KG_SYM(AllGather); KG_SYM(AllReduce); KG_SYM(GetErrorString);
#undef KG_SYM
    r.ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.GroupStart && r.GroupEnd && r.Send && r.Recv && r.AllGather && r.AllReduce && r.GetErrorString;
    return r;
}

// RCCL's two bootstrap calls (ncclGetUniqueId, ncclCommInitRank) open sockets and look for network interfaces, and have been seen not
// to come back on a box (round 5: one `--gpus 1` run of 200 sat in there for its caller's whole 300 s).  They run on a thread of their
// own; the caller waits KATGPU_COMM_INIT_TIMEOUT_S (default 120 s) and then reports an error instead of hanging -- the thread is left
// behind (it owns its state through the shared_ptr), the process is about to fail anyway.
static const double g_comm_init_timeout_s = getenv("KATGPU_COMM_INIT_TIMEOUT_S") ? std::max(1.0, atof(getenv("KATGPU_COMM_INIT_TIMEOUT_S"))) : 120.0;
struct BootCall { std::mutex mu; std::condition_variable cv; bool done = false; ncclResult_t r = ncclSuccess; ncclUniqueId id; ncclComm_t comm = nullptr; };
// false: the call has not returned within the limit
template <typename F>
static bool rccl_boot_call(int device, F&& f, std::shared_ptr<BootCall> st) {
    std::thread([device, f, st]() {
        (void)hipSetDevice(device);
        const ncclResult_t r = f(*st);
        std::lock_guard<std::mutex> lk(st->mu);
        st->r = r; st->done = true;
        st->cv.notify_all();
    }).detach();
    std::unique_lock<std::mutex> lk(st->mu);
    return st->cv.wait_for(lk, std::chrono::duration<double>(g_comm_init_timeout_s), [&] { return st->done; });
}

// ---- the id ranks share: [magic | 16 bytes of token (names the /dev/shm objects) | has_rccl | ncclUniqueId] ----
constexpr uint32_t ID_MAGIC = 0x4B474331;      // "KGC1"
struct CommId { uint32_t magic; uint32_t has_rccl; char token[24]; ncclUniqueId nccl; };
static_assert(sizeof(CommId) <= KATGPU_COMM_ID_BYTES, "id");

// A wait for peers -- at a barrier, for a transfer -- ends with an error (through katgpu_last_error, not a hang) when a peer is DEAD:
// its heartbeat has not moved for this long.  Not a bound on how long a healthy peer may take to get there.
static const double g_comm_timeout_ms = 1e3 * (getenv("KATGPU_COMM_TIMEOUT_S") ? std::max(0.5, atof(getenv("KATGPU_COMM_TIMEOUT_S"))) : 60.0);
// optional: no single wait longer than this, whatever the heartbeats say (0: unbounded)
static const double g_comm_gone_grace_ms = 1e3 * (getenv("KATGPU_COMM_GONE_GRACE_S") ? std::max(0.0, atof(getenv("KATGPU_COMM_GONE_GRACE_S"))) : 5.0);
// (read at the first wait, not when the library is loaded: the host binary gives it a finite default in main(), host/kat_main.cc)
static double comm_max_wait_ms() { static const double v = 1e3 * (getenv("KATGPU_COMM_MAX_WAIT_S") ? std::max(0.0, atof(getenv("KATGPU_COMM_MAX_WAIT_S"))) : 0.0); return v; }
constexpr int BEAT_PERIOD_MS = 50;
constexpr size_t MAILBOX = 64 * 1024;                      // a rank's mailbox in the rendezvous block

}  // namespace

// ---- rendezvous block in /dev/shm: a sense-reversing barrier and a small mailbox per rank ----
struct ShmHeader {
    std::atomic<uint32_t> arrived;
    std::atomic<uint32_t> generation;
    std::atomic<uint32_t> attached;
    uint32_t world;
    std::atomic<uint32_t> aborted;   // a rank that fails inside a collective raises it: its peers leave their barriers with an error instead of waiting for ever
    uint32_t pad_[11];               // (the heartbeats start on a cache line of their own)
};
struct RankBeat { std::atomic<uint64_t> beat; std::atomic<uint32_t> gone; uint32_t pad_[13]; };   // one cache line per rank: its heartbeat; gone: it has left (katgpu_comm_free)
static_assert(sizeof(ShmHeader) == 64 && sizeof(RankBeat) == 64, "shared block layout");

int comm_fail(katgpu_comm* m, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (m && m->ctx) m->ctx->err = buf;
    if (m && m->hdr) m->hdr->aborted.store(1, std::memory_order_release);      // the peers are, or will be, waiting for this rank
    return code;
}
#define NCCLCHK(m, expr)                                                                                               \
    do {                                                                                                               \
        ncclResult_t _r = (expr);                                                                                      \
        if (_r != ncclSuccess) return comm_fail((m), KATGPU_ERR_DEVICE, "%s: %s", #expr, rccl().GetErrorString(_r));  \
    } while (0)

static std::string shm_name(const std::string& token, const char* what, uint64_t seq = 0, int a = 0, int b = 0, int idx = 0) {
    char buf[176];
    snprintf(buf, sizeof buf, "/dev/shm/katgpu-%s-%s-%llu-%d-%d-%d", token.c_str(), what, (unsigned long long)seq, a, b, idx);
    return buf;
}

namespace {
// What a waiting rank knows of its peers' health: each peer's last heartbeat value and when it was last seen to move.
struct Liveness {
    katgpu_comm* m; std::vector<uint64_t> last; std::vector<double> moved, gone_at; double t0; char why[256];
    explicit Liveness(katgpu_comm* m_) : m(m_), last((size_t)m_->world, 0), moved((size_t)m_->world, now_ms()), gone_at((size_t)m_->world, 0.0), t0(now_ms()) {
        why[0] = 0;
        for (int r = 0; r < m->world; ++r) last[r] = m->beats[r].beat.load(std::memory_order_relaxed);
    }
    // false: this wait should end with an error (`why`): a peer failed, left, or its heartbeat stands still; or the optional wall-clock
    // bound.  The caller looks once more at what it waits for before it gives up (a peer may leave right after it did its part).
    bool ok() {
        if (m->hdr->aborted.load(std::memory_order_acquire)) { snprintf(why, sizeof why, "a peer rank failed (rank %d gives up)", m->rank); return false; }
        const double now = now_ms();
        for (int r = 0; r < m->world; ++r) {
            if (r == m->rank) continue;
            const uint64_t b = m->beats[r].beat.load(std::memory_order_relaxed);
            if (b != last[r]) { last[r] = b; moved[r] = now; continue; }
            // A peer that has LEFT (katgpu_comm_free) is not yet a failure: a rank that finished its side of the last collective may free
            // its communicator while a slower rank's transfer is still landing (ncclAllReduce returns per rank).  It becomes one when what
            // this rank waits for has not happened a grace period later (KATGPU_COMM_GONE_GRACE_S, 5 s).
            if (m->beats[r].gone.load(std::memory_order_acquire)) {
                if (gone_at[r] == 0.0) gone_at[r] = now;
                if (now - gone_at[r] > g_comm_gone_grace_ms) { snprintf(why, sizeof why, "rank %d has left the communicator while rank %d waits for it", r, m->rank); return false; }
                continue;
            }
            if (now - moved[r] > g_comm_timeout_ms) {
                snprintf(why, sizeof why, "no sign of life from rank %d for %.0f s (rank %d gives up; KATGPU_COMM_TIMEOUT_S)", r, (now - moved[r]) / 1e3, m->rank);
                return false;
            }
        }
        if (comm_max_wait_ms() > 0 && now - t0 > comm_max_wait_ms()) { snprintf(why, sizeof why, "rank %d waited %.0f s (KATGPU_COMM_MAX_WAIT_S)", m->rank, (now - t0) / 1e3); return false; }
        return true;
    }
};
}  // namespace

// every rank of the communicator: wait until all have arrived -- or until a peer has failed (ShmHeader::aborted) or died (its heartbeat)
int shm_barrier(katgpu_comm* m) {
    if (m->world == 1) return KATGPU_OK;
    if (m->hdr->aborted.load(std::memory_order_acquire)) return comm_fail(m, KATGPU_ERR_DEVICE, "a peer rank failed (rank %d leaves the barrier)", m->rank);
    const uint32_t gen = m->hdr->generation.load(std::memory_order_acquire);
    if (m->hdr->arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == (uint32_t)m->world) {
        m->hdr->arrived.store(0, std::memory_order_relaxed);
        m->hdr->generation.store(gen + 1, std::memory_order_release);
    } else {
        Liveness live(m);
        for (uint32_t spins = 0; m->hdr->generation.load(std::memory_order_acquire) == gen; ++spins) {
            if (spins <= 1000) continue;
            if ((spins & 255) == 0 && !live.ok()) {
                if (m->hdr->generation.load(std::memory_order_acquire) != gen) break;          // everyone did arrive (and one has left since)
                return comm_fail(m, KATGPU_ERR_DEVICE, "barrier: %s", live.why);
            }
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
    }
    return KATGPU_OK;
}
// wait for the transport stream (or an event on it) the same way: a collective whose peer never posts its side would sit in
// hipStreamSynchronize for ever
int comm_wait(katgpu_comm* m, hipEvent_t ev /* or null: the whole stream */, const char* what) {
    Liveness live(m);
    auto query = [&]() { return ev ? hipEventQuery(ev) : hipStreamQuery(m->stream); };
    for (uint32_t spins = 0;; ++spins) {
        const hipError_t e = query();
        if (e == hipSuccess) return KATGPU_OK;
        if (e != hipErrorNotReady) return comm_fail(m, KATGPU_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
        if (spins < 2000) continue;
        if ((spins & 255) == 0 && m->hdr && !live.ok()) {
            if (query() == hipSuccess) return KATGPU_OK;
            return comm_fail(m, KATGPU_ERR_DEVICE, "%s: %s", what, live.why);
        }
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

// small host values through the mailboxes: out[r * n .. ) = rank r's n bytes
static int host_allgather(katgpu_comm* m, const void* mine, size_t n, void* out) {
    if (n > MAILBOX) return comm_fail(m, KATGPU_ERR_INVALID_ARG, "host_allgather: %zu bytes per rank", n);
    if (m->world == 1) { memcpy(out, mine, n); return KATGPU_OK; }
    memcpy(m->boxes + (size_t)m->rank * MAILBOX, mine, n);
    int rc = shm_barrier(m);
    if (rc) return rc;
    for (int r = 0; r < m->world; ++r) memcpy((uint8_t*)out + (size_t)r * n, m->boxes + (size_t)r * MAILBOX, n);
    return shm_barrier(m);
}

static int ensure_host_stage(katgpu_comm* m, size_t bytes) {
    if (m->host_stage_bytes >= bytes) return KATGPU_OK;
    if (m->host_stage) hipHostFree(m->host_stage);
    m->host_stage = nullptr; m->host_stage_bytes = 0;
    if (hipHostMalloc((void**)&m->host_stage, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return comm_fail(m, KATGPU_ERR_NOMEM, "pinned staging of %zu bytes", bytes); }
    m->host_stage_bytes = bytes;
    return KATGPU_OK;
}

// (SHM: every send is a file in /dev/shm that its receiver reads and the sender removes)
int transfer(katgpu_comm* m, const std::vector<CommMsg>& sends, const std::vector<CommMsg>& recvs, hipEvent_t ev) {
    katgpu_ctx* c = m->ctx;
    if (m->use_rccl) {
        bool any = false;
        for (auto& s : sends) any = any || s.bytes;
        for (auto& r : recvs) any = any || r.bytes;
        if (any) {
            NCCLCHK(m, rccl().GroupStart());
            for (auto& s : sends) if (s.bytes) NCCLCHK(m, rccl().Send(s.dev, s.bytes, ncclUint8, s.peer, m->nccl, m->stream));
            for (auto& r : recvs) if (r.bytes) NCCLCHK(m, rccl().Recv(r.dev, r.bytes, ncclUint8, r.peer, m->nccl, m->stream));
            NCCLCHK(m, rccl().GroupEnd());
        }
        for (auto& s : sends) m->bytes_sent += s.bytes;
        if (ev) HIPCHK(c, hipEventRecord(ev, m->stream));
        return KATGPU_OK;
    }
    const uint64_t seq = m->seq++;
    size_t biggest = 0;
    for (auto& s : sends) biggest = std::max(biggest, s.bytes);
    for (auto& r : recvs) biggest = std::max(biggest, r.bytes);
    int rc = ensure_host_stage(m, std::max<size_t>(biggest, 4096));
    if (rc) return rc;
    // (a group may carry several messages for one peer -- keys, then counts: the n-th to a peer meets the n-th from it)
    std::vector<int> nth((size_t)m->world, 0);
    for (auto& s : sends) {
        const int idx = nth[s.peer]++;
        if (!s.bytes) continue;
        if (hipMemcpy(m->host_stage, s.dev, s.bytes, hipMemcpyDeviceToHost) != hipSuccess) return comm_fail(m, KATGPU_ERR_DEVICE, "staging a message for rank %d", s.peer);
        const std::string name = shm_name(m->token, "x", seq, m->rank, s.peer, idx);
        const int fd = ::open(name.c_str(), O_CREAT | O_TRUNC | O_WRONLY, 0600);
        if (fd < 0) return comm_fail(m, KATGPU_ERR_IO, "cannot create %s", name.c_str());
        size_t off = 0;
        while (off < s.bytes) { const ssize_t w = ::write(fd, m->host_stage + off, s.bytes - off); if (w <= 0) { ::close(fd); return comm_fail(m, KATGPU_ERR_IO, "short write to %s", name.c_str()); } off += (size_t)w; }
        ::close(fd);
        m->bytes_sent += s.bytes;
    }
    rc = shm_barrier(m);
    if (rc) return rc;
    std::fill(nth.begin(), nth.end(), 0);
    for (auto& r : recvs) {
        const int idx = nth[r.peer]++;
        if (!r.bytes) continue;
        const std::string name = shm_name(m->token, "x", seq, r.peer, m->rank, idx);
        const int fd = ::open(name.c_str(), O_RDONLY);
        if (fd < 0) return comm_fail(m, KATGPU_ERR_IO, "cannot open %s", name.c_str());
        size_t off = 0;
        while (off < r.bytes) { const ssize_t g = ::read(fd, m->host_stage + off, r.bytes - off); if (g <= 0) { ::close(fd); return comm_fail(m, KATGPU_ERR_IO, "short read from %s", name.c_str()); } off += (size_t)g; }
        ::close(fd);
        ::unlink(name.c_str());
        if (hipMemcpy(r.dev, m->host_stage, r.bytes, hipMemcpyHostToDevice) != hipSuccess) return comm_fail(m, KATGPU_ERR_DEVICE, "unstaging a message from rank %d", r.peer);
    }
    return shm_barrier(m);
}
int transfer_wait(katgpu_comm* m, hipEvent_t ev) {
    if (m->use_rccl && ev) return comm_wait(m, ev, "exchange");
    return KATGPU_OK;
}

int allgather_u64(katgpu_comm* m, const uint64_t* mine, size_t n, uint64_t* out) {
    katgpu_ctx* c = m->ctx;
    if (m->world == 1) { memcpy(out, mine, n * 8); return KATGPU_OK; }
    if (!m->use_rccl && n * 8 <= MAILBOX) return host_allgather(m, mine, n * 8, out);
    uint64_t* d = nullptr;
    HIPCHK(c, hipMalloc((void**)&d, (size_t)(m->world + 1) * n * 8));
    int rc = KATGPU_OK;
    if (hipMemcpy(d, mine, n * 8, hipMemcpyHostToDevice) != hipSuccess) rc = comm_fail(m, KATGPU_ERR_DEVICE, "allgather upload");
    if (!rc && m->use_rccl) {
        ncclResult_t r = rccl().AllGather(d, d + n, n, ncclUint64, m->nccl, m->stream);
        if (r != ncclSuccess) rc = comm_fail(m, KATGPU_ERR_DEVICE, "ncclAllGather: %s", rccl().GetErrorString(r));
        else rc = comm_wait(m, nullptr, "allgather");
    } else if (!rc) {
        std::vector<CommMsg> s, rv;
        for (int p = 0; p < m->world; ++p) {
            if (p == m->rank) { if (hipMemcpy(d + n + (size_t)p * n, d, n * 8, hipMemcpyDeviceToDevice) != hipSuccess) rc = KATGPU_ERR_DEVICE; continue; }
            s.push_back({p, d, n * 8});
            rv.push_back({p, d + n + (size_t)p * n, n * 8});
        }
        if (!rc) rc = transfer(m, s, rv, nullptr);
    }
    if (!rc && hipMemcpy(out, d + n, (size_t)m->world * n * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = comm_fail(m, KATGPU_ERR_DEVICE, "allgather download");
    hipFree(d);
    return rc;
}

void comm_abort(katgpu_comm* m) { if (m->hdr) m->hdr->aborted.store(1, std::memory_order_release); }

// ---- all go on, or none does (kg_comm.hpp) ----
int comm_agree(katgpu_comm* m, uint64_t mine, int* who, uint64_t* what) {
    std::vector<uint64_t> all((size_t)m->world, 0);
    const int rc = allgather_u64(m, &mine, 1, all.data());
    *who = -1;
    for (int p = m->world - 1; p >= 0 && !rc; --p) if (all[p]) { *who = p; if (what) *what = all[p]; }
    return rc;
}

int comm_agree_to_start(katgpu_comm* m, int rc, const std::function<int(int who, int code)>& peer_error) {
    const std::string err_local = rc ? m->ctx->err : std::string();
    int who = -1;
    uint64_t what = 0;                                            // 1: no memory, 2: anything else
    const int crc = comm_agree(m, rc == KATGPU_ERR_NOMEM ? 1 : rc ? 2 : 0, &who, &what);
    if (crc) return rc ? rc : crc;                                // (the communicator itself failed: its waits have ended on every rank)
    if (who < 0) return KATGPU_OK;
    if (rc) { m->ctx->err = err_local; return rc; }
    return peer_error(who, what == 1 ? KATGPU_ERR_NOMEM : KATGPU_ERR_DEVICE);
}

int comm_agree_done(katgpu_comm* m, int rc, const char* rank_failed_fmt) {
    const std::string err_mine = rc ? m->ctx->err : std::string();
    if (rc) comm_abort(m);
    int who = -1;
    const int crc = comm_agree(m, rc ? 1 : 0, &who);
    if (rc) { m->ctx->err = err_mine; return rc == KATGPU_ERR_NOMEM ? KATGPU_ERR_DEVICE : rc; }   // (not the collective one: the peers get an error too)
    if (crc) return crc;
    if (who >= 0) return fail(m->ctx, KATGPU_ERR_DEVICE, rank_failed_fmt, who);
    return KATGPU_OK;
}

std::function<int(int who, int code)> gathered_peer_error(katgpu_comm* m, katgpu_ctx* c, const char* name, const char* room_fmt, size_t room) {
    return [=](int p, int code) {
        if (code != KATGPU_ERR_NOMEM) return fail(c, code, "%s: rank %d could not read its table", name, p);
        return fail(c, code, (std::string("%s: rank %d of %d has no device memory for ") + room_fmt).c_str(), name, p, m->world, room);
    };
}

// ---- the same call on every rank (kg_comm.hpp) ----
// every start and length, in order, folded into one word
static uint64_t records_checksum(const CallRecords& recs) {
    uint64_t h = 0x9E3779B97F4A7C15ULL;
    auto fold = [&](uint64_t x) { h ^= x; h *= 0xFF51AFD7ED558CCDULL; h ^= h >> 32; };
    for (size_t r = 0; r < recs.n; ++r) { fold(recs.start[r]); fold(recs.len[r]); }
    return h;
}

int comm_agree_on_call(katgpu_comm* m, katgpu_ctx* c, const char* name, size_t n, uint32_t k, const CallRecords* recs, bool unusable, const char* unusable_what,
                       const CallWords* extra) {
    enum { N, K, N_REC, CHECKSUM, UNUSABLE, EXTRA };                // a rank's words
    typedef unsigned long long ull;
    const size_t n_extra = extra ? extra->n : 0, W = EXTRA + n_extra;
    std::vector<uint64_t> mine(W, 0), all((size_t)m->world * W, 0);
    mine[N] = n; mine[K] = k; mine[N_REC] = recs ? recs->n : 0; mine[UNUSABLE] = unusable;
    if (recs && !unusable) mine[CHECKSUM] = records_checksum(*recs);
    for (size_t i = 0; i < n_extra; ++i) mine[EXTRA + i] = extra->words[i];
    const int crc = allgather_u64(m, mine.data(), W, all.data());
    if (crc) return crc;
    const uint64_t* r0 = all.data();
    for (int p = 0; p < m->world; ++p)
        if (all[(size_t)p * W + UNUSABLE]) return fail(c, KATGPU_ERR_INVALID_ARG, "%s: rank %d %s", name, p, unusable_what);
    for (int p = 0; p < m->world; ++p) {
        const uint64_t* a = &all[(size_t)p * W];
        if (a[N] != r0[N] || a[N_REC] != r0[N_REC] || a[K] != r0[K]) {
            if (recs) return fail(c, KATGPU_ERR_INVALID_ARG, "%s: the ranks disagree: rank 0 has %llu bases in %llu records at k = %llu, rank %d %llu in %llu at k = %llu", name,
                                  (ull)r0[N], (ull)r0[N_REC], (ull)r0[K], p, (ull)a[N], (ull)a[N_REC], (ull)a[K]);
            return fail(c, KATGPU_ERR_INVALID_ARG, "%s: the ranks disagree: rank 0 has %llu bases at k = %llu, rank %d %llu at k = %llu", name, (ull)r0[N], (ull)r0[K], p, (ull)a[N], (ull)a[K]);
        }
        if (a[CHECKSUM] != r0[CHECKSUM]) return fail(c, KATGPU_ERR_INVALID_ARG, "%s: the ranks disagree: rank %d's %llu records are not where rank 0's are", name, p, (ull)a[N_REC]);
        if (n_extra && memcmp(a + EXTRA, r0 + EXTRA, n_extra * sizeof(uint64_t))) return fail(c, KATGPU_ERR_INVALID_ARG, "%s: the ranks disagree: rank %d's %s", name, p, extra->differ);
    }
    return KATGPU_OK;
}

// ------------------------------------------------------------------ the communicator ------------------

extern "C" int katgpu_comm_unique_id(void* id_out) {
    if (!id_out) return KATGPU_ERR_INVALID_ARG;
    CommId id{};
    id.magic = ID_MAGIC;
    FILE* f = fopen("/dev/urandom", "rb");
    uint8_t rnd[10] = {0};
    if (f) { if (fread(rnd, 1, sizeof rnd, f) != sizeof rnd) rnd[0] = (uint8_t)getpid(); fclose(f); }
    snprintf(id.token, sizeof id.token, "%02x%02x%02x%02x%02x%02x%02x%02x%02x%02x", rnd[0], rnd[1], rnd[2], rnd[3], rnd[4], rnd[5], rnd[6], rnd[7], rnd[8], rnd[9]);
    const char* tr = getenv("KATGPU_COMM_TRANSPORT");
    if (!(tr && !strcmp(tr, "shm")) && rccl().ok) {
        int dev = 0; (void)hipGetDevice(&dev);
        auto st = std::make_shared<BootCall>();
        if (!rccl_boot_call(dev, [](BootCall& b) { return rccl().GetUniqueId(&b.id); }, st)) {
            fprintf(stderr, "[katgpu] ncclGetUniqueId did not return within %.0f s (KATGPU_COMM_INIT_TIMEOUT_S)\n", g_comm_init_timeout_s);
            return KATGPU_ERR_DEVICE;
        }
        if (st->r == ncclSuccess) { id.nccl = st->id; id.has_rccl = 1; }
    }
    memset(id_out, 0, KATGPU_COMM_ID_BYTES);
    memcpy(id_out, &id, sizeof id);
    return KATGPU_OK;
}

extern "C" void katgpu_comm_free(katgpu_comm* m) {
    if (!m) return;
    if (m->ctx) hipSetDevice(m->ctx->device);
    drop_pending(m);
    if (m->nccl) rccl().CommDestroy(m->nccl);
    for (auto& e : m->ev) if (e) hipEventDestroy(e);
    if (m->stream) hipStreamDestroy(m->stream);
    if (m->host_stage) hipHostFree(m->host_stage);
    if (m->beat_thread.joinable()) { m->beat_stop.store(true); m->beat_thread.join(); }
    if (m->hdr) {
        if (m->beats) m->beats[m->rank].gone.store(1, std::memory_order_release);          // a peer still waiting for this rank learns it at once, not from a silent heartbeat
        const bool last = m->hdr->attached.fetch_sub(1) == 1;
        munmap((void*)m->hdr, m->shm_bytes);
        if (last || m->rank == 0) ::unlink(shm_name(m->token, "hdr").c_str());
    }
    delete m;
}

extern "C" int katgpu_comm_init(katgpu_ctx* c, int rank, int world, const void* id_in, katgpu_comm** out) {
    if (!c || !out || !id_in || world < 1 || rank < 0 || rank >= world || world > (int)MAX_EXCHANGE_PARTS_HOST) return KATGPU_ERR_INVALID_ARG;
    *out = nullptr;
    CommId id;
    memcpy(&id, id_in, sizeof id);
    if (id.magic != ID_MAGIC) return fail(c, KATGPU_ERR_INVALID_ARG, "katgpu_comm_init: not an id made by katgpu_comm_unique_id");
    HIPCHK(c, hipSetDevice(c->device));
    katgpu_comm* m = new katgpu_comm();
    m->ctx = c; m->rank = rank; m->world = world;
    id.token[sizeof id.token - 1] = 0;
    m->token = id.token;
    // the rendezvous block: every rank maps it (rank order does not matter: O_CREAT, then ftruncate to the same size)
    m->shm_bytes = sizeof(ShmHeader) + (size_t)world * sizeof(RankBeat) + (size_t)world * MAILBOX;
    const std::string hname = shm_name(m->token, "hdr");
    const int fd = ::open(hname.c_str(), O_CREAT | O_RDWR, 0600);
    if (fd < 0 || ftruncate(fd, (off_t)m->shm_bytes) != 0) { if (fd >= 0) ::close(fd); delete m; return fail(c, KATGPU_ERR_IO, "cannot create %s", hname.c_str()); }
    void* p = mmap(nullptr, m->shm_bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    ::close(fd);
    if (p == MAP_FAILED) { delete m; return fail(c, KATGPU_ERR_IO, "cannot map %s", hname.c_str()); }
    m->hdr = (ShmHeader*)p;                       // (a fresh file is zero-filled: counters start at 0)
    m->beats = (RankBeat*)((uint8_t*)p + sizeof(ShmHeader));
    m->boxes = (uint8_t*)p + sizeof(ShmHeader) + (size_t)world * sizeof(RankBeat);
    // this rank's heartbeat: alive as long as the process is, whatever the main thread is busy with (counting a .gz for minutes)
    m->beats[rank].beat.store(1, std::memory_order_relaxed);
    m->beat_thread = std::thread([m, rank]() {
        while (!m->beat_stop.load(std::memory_order_relaxed)) {
            m->beats[rank].beat.fetch_add(1, std::memory_order_relaxed);
            std::this_thread::sleep_for(std::chrono::milliseconds(BEAT_PERIOD_MS));
        }
    });
    m->hdr->attached.fetch_add(1);
    // wait for everyone (bounded: a rank that never shows up must not hang the others for ever)
    const double t0 = now_ms();
    while (m->hdr->attached.load() < (uint32_t)world) {
        if (now_ms() - t0 > 120e3) {
            const int seen = (int)m->hdr->attached.load();        // (before the block is unmapped)
            katgpu_comm_free(m);
            return fail(c, KATGPU_ERR_DEVICE, "katgpu_comm_init: %d rank(s) of %d showed up within 120 s", seen, world);
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    {   // (every way out from here on gives the communicator back: katgpu_comm_free copes with a half-made one)
        hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
        for (auto& ev : m->ev) if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) { katgpu_comm_free(m); return fail(c, KATGPU_ERR_DEVICE, "katgpu_comm_init: %s", hipGetErrorString(e)); }
    }
    // which devices the ranks run on: ranks that share one cannot have RCCL (it refuses two ranks on a device) and stage through /dev/shm;
    // ranks on devices of their own must not end up there by accident
    int rc = KATGPU_OK;
    {
        char mine_id[64] = {0};
        if (hipDeviceGetPCIBusId(mine_id, (int)sizeof mine_id - 1, c->device) != hipSuccess) { (void)hipGetLastError(); snprintf(mine_id, sizeof mine_id, "device-%d", c->device); }
        std::vector<char> ids((size_t)world * sizeof mine_id);
        rc = host_allgather(m, mine_id, sizeof mine_id, ids.data());
        if (rc) { katgpu_comm_free(m); return rc; }
        std::vector<std::string> uniq;
        for (int r = 0; r < world; ++r) { std::string d(ids.data() + (size_t)r * sizeof mine_id); if (std::find(uniq.begin(), uniq.end(), d) == uniq.end()) uniq.push_back(d); }
        m->distinct_devices = (int)uniq.size();
    }
    // transport: RCCL when every rank can have it
    const char* tr = getenv("KATGPU_COMM_TRANSPORT");
    const bool asked_shm = tr && !strcmp(tr, "shm");
    const bool want_rccl = !asked_shm && id.has_rccl && rccl().ok;
    uint32_t mine = 0;
    if (want_rccl) {
        auto st = std::make_shared<BootCall>();
        st->id = id.nccl;
        if (!rccl_boot_call(c->device, [world, rank](BootCall& b) { return rccl().CommInitRank(&b.comm, world, b.id, rank); }, st)) {
            m->beats[rank].gone.store(1, std::memory_order_release);
            // (the communicator is NOT taken apart: the thread inside RCCL may still touch what it was given; the process is to end)
            return fail(c, KATGPU_ERR_DEVICE, "katgpu_comm_init: ncclCommInitRank did not return within %.0f s on rank %d of %d (KATGPU_COMM_INIT_TIMEOUT_S)", g_comm_init_timeout_s, rank, world);
        }
        const ncclResult_t r = st->r;
        if (r == ncclSuccess) { m->nccl = st->comm; mine = 1; }
        else { m->nccl = nullptr; m->transport_note = std::string("RCCL refused to initialise (") + rccl().GetErrorString(r) + ")"; (void)hipGetLastError(); }
    } else m->transport_note = asked_shm ? "KATGPU_COMM_TRANSPORT=shm" : (id.has_rccl ? "librccl could not be loaded here" : "no RCCL id (librccl missing where the id was made)");
    std::vector<uint32_t> all((size_t)world);
    rc = host_allgather(m, &mine, sizeof mine, all.data());
    if (rc) { katgpu_comm_free(m); return rc; }
    m->use_rccl = true;
    for (uint32_t v : all) m->use_rccl = m->use_rccl && v;
    if (!m->use_rccl && m->nccl) { rccl().CommDestroy(m->nccl); m->nccl = nullptr; if (m->transport_note.empty()) m->transport_note = "a peer could not initialise RCCL"; }
    if (tr && !strcmp(tr, "rccl") && !m->use_rccl) { std::string why = m->transport_note; katgpu_comm_free(m); return fail(c, KATGPU_ERR_DEVICE, "KATGPU_COMM_TRANSPORT=rccl: %s", why.c_str()); }
    // no silent fall-back between devices: /dev/shm staging is for ranks that share a device (or for whoever asked for it by name)
    if (!m->use_rccl && world > 1 && m->distinct_devices > 1 && !asked_shm && !getenv("KATGPU_COMM_ALLOW_SHM")) {
        std::string why = m->transport_note;
        const int nd = m->distinct_devices;
        katgpu_comm_free(m);
        return fail(c, KATGPU_ERR_DEVICE, "katgpu_comm_init: %d ranks on %d devices, and RCCL is not to be had (%s): refusing to stage the exchange through /dev/shm "
                    "(KATGPU_COMM_ALLOW_SHM=1 or KATGPU_COMM_TRANSPORT=shm to take it knowingly)", world, nd, why.c_str());
    }
    if (g_trace) fprintf(stderr, "[katgpu] comm: rank %d of %d, transport %s%s%s\n", rank, world, m->use_rccl ? "RCCL" : "SHM (staged through /dev/shm)", m->transport_note.empty() ? "" : ": ", m->transport_note.c_str());
    *out = m;
    return KATGPU_OK;
}

extern "C" int katgpu_comm_rank(const katgpu_comm* m) { return m ? m->rank : -1; }
extern "C" int katgpu_comm_world(const katgpu_comm* m) { return m ? m->world : 0; }
extern "C" const char* katgpu_comm_transport(const katgpu_comm* m) { return !m ? "" : m->use_rccl ? "rccl" : "shm"; }
extern "C" const char* katgpu_comm_transport_note(const katgpu_comm* m) { return m ? m->transport_note.c_str() : ""; }
extern "C" int katgpu_comm_distinct_devices(const katgpu_comm* m) { return m ? m->distinct_devices : 0; }

extern "C" int katgpu_comm_barrier(katgpu_comm* m) {
    if (!m) return KATGPU_ERR_INVALID_ARG;
    HIPCHK(m->ctx, hipSetDevice(m->ctx->device));
    HIPCHK(m->ctx, hipStreamSynchronize(m->ctx->stream));
    return shm_barrier(m);
}

extern "C" int katgpu_comm_wire(katgpu_comm* m, uint64_t* records_sent, uint64_t* record_bytes_sent, int* packed) {
    if (!m) return KATGPU_ERR_INVALID_ARG;
    if (records_sent) *records_sent = m->records_sent;
    if (record_bytes_sent) *record_bytes_sent = m->record_bytes_sent;
    if (packed) *packed = m->wire_packed ? 1 : 0;
    return KATGPU_OK;
}

extern "C" int katgpu_comm_stats(katgpu_comm* m, double* ms_extract, double* ms_exchange, double* ms_merge, double* ms_allreduce, uint64_t* bytes_sent, uint64_t* merge_launches) {
    if (!m) return KATGPU_ERR_INVALID_ARG;
    if (ms_extract) *ms_extract = m->ms_extract;
    if (ms_exchange) *ms_exchange = m->ms_exchange;
    if (ms_merge) *ms_merge = m->ms_merge;
    if (ms_allreduce) *ms_allreduce = m->ms_allreduce;
    if (bytes_sent) *bytes_sent = m->bytes_sent;
    if (merge_launches) *merge_launches = m->merge_launches;
    return KATGPU_OK;
}

// Sum of `n` u64 over all ranks, in place, every rank gets the result: the small results of the reducers (hist 80 KB, gcp 216 KB,
// comp 8 MB + counters) -- what mergeThreadedMatricies / ThreadedCompCounters::merge / Histogram::merge do for threads.
extern "C" int katgpu_allreduce_u64(katgpu_comm* m, uint64_t* buf, size_t n) {
    if (!m || (n && !buf)) return KATGPU_ERR_INVALID_ARG;
    if (m->world == 1 || n == 0) return KATGPU_OK;
    katgpu_ctx* c = m->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    const double t0 = now_ms();
    int rc = KATGPU_OK;
    if (m->use_rccl) {
        uint64_t* d = nullptr;
        HIPCHK(c, hipMalloc((void**)&d, n * 8));
        if (hipMemcpy(d, buf, n * 8, hipMemcpyHostToDevice) != hipSuccess) rc = comm_fail(m, KATGPU_ERR_DEVICE, "allreduce upload");
        if (!rc) {
            ncclResult_t r = rccl().AllReduce(d, d, n, ncclUint64, ncclSum, m->nccl, m->stream);
            if (r != ncclSuccess) rc = comm_fail(m, KATGPU_ERR_DEVICE, "ncclAllReduce: %s", rccl().GetErrorString(r));
            else if ((rc = comm_wait(m, nullptr, "allreduce")) == KATGPU_OK && hipMemcpy(buf, d, n * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = comm_fail(m, KATGPU_ERR_DEVICE, "allreduce");
        }
        hipFree(d);
    } else {
        // every rank writes its vector, reads all of them (host memory only: the vectors are small)
        const uint64_t seq = m->seq++;
        const std::string mine = shm_name(m->token, "r", seq, m->rank, 0);
        FILE* f = fopen(mine.c_str(), "wb");
        if (!f || fwrite(buf, 8, n, f) != n) rc = comm_fail(m, KATGPU_ERR_IO, "cannot write %s", mine.c_str());
        if (f) fclose(f);
        if (!rc) rc = shm_barrier(m);                            // (a rank that could not write has raised the abort flag: its peers leave here too)
        std::vector<uint64_t> other(n);
        for (int r = 0; r < m->world && !rc; ++r) {
            if (r == m->rank) continue;
            const std::string name = shm_name(m->token, "r", seq, r, 0);
            FILE* g = fopen(name.c_str(), "rb");
            if (!g || fread(other.data(), 8, n, g) != n) rc = comm_fail(m, KATGPU_ERR_IO, "cannot read %s", name.c_str());
            if (g) fclose(g);
            if (!rc) for (size_t i = 0; i < n; ++i) buf[i] += other[i];
        }
        if (!rc) rc = shm_barrier(m);
        ::unlink(mine.c_str());
    }
    m->ms_allreduce += now_ms() - t0;
    return rc;
}
