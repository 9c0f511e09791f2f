// include/mobgt_checkins.h: check-in sessions from a raw check-in log.
//
// Everything but the cut is one thread per record, per session or per user: integer atomics into counters (records per user and
// POI, members per session, kept sessions per user, the first output position of a POI and of a category) and plain stores at
// positions the caller's prefix sums fixed.  The cut is sequential per user -- a full session forces a new one whatever the gap --
// and runs as a scan: cut_kernel, one wave per user, below.
//
// Every id is checked before it is an index, and so is every index read from a buffer (a key's log position, a prefix sum's
// value); what fails is skipped and reported in status[0].  No workgroup reads what another writes in the same launch, except
// through integer atomics whose results are read by a LATER launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mobgt_checkins.h"

namespace {

constexpr int TPB = 256;
constexpr int WAVE = MOBGT_CHECKINS_WAVE;
constexpr int WAVES = TPB / WAVE;
constexpr int FILL_BLOCKS = 2048;
constexpr int64_t NOKEY = MOBGT_CHECKINS_NOKEY;

__device__ inline int64_t tid() { return (int64_t)blockIdx.x * TPB + threadIdx.x; }

unsigned blocks(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

unsigned fill_blocks(int64_t n) {
    const int64_t b = (n + TPB - 1) / TPB;
    return (unsigned)(b < 1 ? 1 : b < FILL_BLOCKS ? b : FILL_BLOCKS);
}

// ---- step 1 -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void count_start_kernel(int64_t n, int64_t U0, int64_t P0, int32_t* __restrict__ ucnt,
                                                          int32_t* __restrict__ pcnt, int32_t* __restrict__ ufirst,
                                                          int32_t* __restrict__ status) {
    const int64_t stride = (int64_t)gridDim.x * TPB;
    for (int64_t i = tid(); i < n; i += stride) {
        if (i < U0) {
            ucnt[i] = 0;
            ufirst[i] = INT32_MAX;
        }
        if (i < P0) pcnt[i] = 0;
        if (i == 0) status[0] = 0;
    }
}

__device__ inline int id_bits(int64_t u, int64_t p, int64_t c, int64_t U0, int64_t P0, int64_t C0) {
    return (u >= 1 && u <= U0 ? 0 : MOBGT_CHECKINS_SBADUSER) | (p >= 1 && p <= P0 ? 0 : MOBGT_CHECKINS_SBADPOI) |
           (c >= 1 && c <= C0 ? 0 : MOBGT_CHECKINS_SBADCAT);
}

__global__ __launch_bounds__(TPB) void count_kernel(const int32_t* __restrict__ user, const int32_t* __restrict__ poi,
                                                    const int32_t* __restrict__ cat, int64_t N, int64_t U0, int64_t P0, int64_t C0,
                                                    int32_t* __restrict__ ucnt, int32_t* __restrict__ pcnt, int32_t* __restrict__ ufirst,
                                                    int32_t* __restrict__ status) {
    const int64_t i = tid();
    if (i >= N) return;
    const int64_t u = user[i], p = poi[i];
    const int bad = id_bits(u, p, cat[i], U0, P0, C0);
    if (bad) {
        atomicOr(status, bad);
        return;
    }
    atomicAdd(&ucnt[u - 1], 1);
    atomicAdd(&pcnt[p - 1], 1);
    atomicMin(&ufirst[u - 1], (int32_t)i);
}

__global__ __launch_bounds__(TPB) void user_key_kernel(const int32_t* __restrict__ ucnt, const int32_t* __restrict__ ufirst, int64_t U0,
                                                       int64_t trace_min, int64_t* __restrict__ ukey) {
    const int64_t u = tid();
    if (u >= U0) return;
    const int64_t c = ucnt[u];
    ukey[u] = c >= 1 && c >= trace_min ? ((int64_t)(INT32_MAX - c) << 32) | (int64_t)ufirst[u] : NOKEY;
}

__global__ __launch_bounds__(TPB) void keys_kernel(const int32_t* __restrict__ user, const int32_t* __restrict__ poi,
                                                   const int32_t* __restrict__ cat, int64_t N, int64_t U0, int64_t P0, int64_t C0,
                                                   const int32_t* __restrict__ urank, int64_t U1, const int32_t* __restrict__ pcnt,
                                                   int64_t global_visit, int64_t* __restrict__ keys) {
    const int64_t i = tid();
    if (i >= N) return;
    const int64_t u = user[i], p = poi[i];
    int64_t key = NOKEY;
    if (!id_bits(u, p, cat[i], U0, P0, C0)) {
        const int64_t r = urank[u - 1];
        if (r >= 0 && r < U1 && pcnt[p - 1] >= global_visit) key = (r << 32) | i;
    }
    keys[i] = key;
}

// ---- step 2: the cut ------------------------------------------------------------------------------------------------------------
// A map f of the session length s in 1 .. 16 onto itself is 16 nibbles: nibble s - 1 holds f(s) - 1.
constexpr uint64_t IDENTITY = 0xFEDCBA9876543210ull;

__device__ inline int apply(uint64_t f, int s) { return (int)((f >> (4 * (s - 1))) & 15) + 1; }

// first f, then g
__device__ inline uint64_t then(uint64_t f, uint64_t g) {
    uint64_t h = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) h |= ((g >> (4 * ((f >> (4 * k)) & 15))) & 15) << (4 * k);
    return h;
}

__device__ inline uint64_t shfl_up64(uint64_t v, int d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d, WAVE), hi = __shfl_up((uint32_t)(v >> 32), d, WAVE);
    return ((uint64_t)hi << 32) | lo;
}

__device__ inline uint64_t shfl64(uint64_t v, int lane) {
    const uint32_t lo = __shfl((uint32_t)v, lane, WAVE), hi = __shfl((uint32_t)(v >> 32), lane, WAVE);
    return ((uint64_t)hi << 32) | lo;
}

// the first j in 0 .. R with keys[j] >= target
__device__ inline int64_t lower_bound(const int64_t* __restrict__ keys, int64_t R, int64_t target) {
    int64_t lo = 0, hi = R;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < target) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Wave w of workgroup b owns user rank b * WAVES + w.  No __syncthreads: the waves of a workgroup share nothing.
__global__ __launch_bounds__(TPB) void cut_kernel(const int64_t* __restrict__ keys, int64_t R, const int64_t* __restrict__ t, int64_t N,
                                                  int64_t U1, int64_t hour_gap_s, int64_t min_gap_s, int session_max,
                                                  int32_t* __restrict__ start, int32_t* __restrict__ member, int32_t* __restrict__ status) {
    const int lane = threadIdx.x % WAVE;
    const int64_t r = (int64_t)blockIdx.x * WAVES + threadIdx.x / WAVE;
    if (r >= U1) return;                                                // (wave-uniform)
    uint64_t append = 0, skip = 0;                                      // s > session_max -> 1 in both (nibble 0)
    for (int k = 0; k < session_max; ++k) {                             // s = k + 1 <= session_max
        append |= (uint64_t)(k + 1) << (4 * k);
        skip |= (uint64_t)k << (4 * k);
    }
    const int64_t lo = lower_bound(keys, R, r << 32), hi = lower_bound(keys, R, (r + 1) << 32);
    int carry_s = 1;                                                    // (not read: the first record is a RESET)
    int64_t carry_t = 0;
    for (int64_t base = lo; base < hi; base += WAVE) {                  // (wave-uniform bounds: every lane takes every shuffle)
        const int64_t j = base + lane;
        bool valid = j < hi;
        int64_t i = valid ? (keys[j] & 0xffffffffll) : 0;
        if (valid && i >= N) {                                          // a key from elsewhere: never an index; the record is dropped
            atomicOr(status, MOBGT_CHECKINS_SBADINDEX);
            start[j] = member[j] = 0;
            valid = false;
        }
        const int64_t tj = valid ? t[i] : 0;
        int64_t tprev = (int64_t)shfl_up64((uint64_t)tj, 1);
        if (lane == 0) tprev = carry_t;
        // 0 RESET, 1 APPEND, 2 SKIP, 3 no record (the identity)
        int kind = 3;
        if (valid) {
            const int64_t g = tj - tprev;
            kind = j == lo || g >= hour_gap_s ? 0 : g >= min_gap_s ? 1 : 2;
        }
        const uint64_t own = kind == 0 ? 0ull : kind == 1 ? append : kind == 2 ? skip : IDENTITY;
        uint64_t f = own;                                               // inclusive scan: records base .. j, in order
#pragma unroll
        for (int d = 1; d < WAVE; d *= 2) {
            const uint64_t before = shfl_up64(f, d);
            if (lane >= d) f = then(before, f);
        }
        uint64_t pre = shfl_up64(f, 1);                                 // the records before j of this chunk
        if (lane == 0) pre = IDENTITY;
        const int s = apply(pre, carry_s);                              // the session length before record j
        if (valid) {
            const bool st = kind == 0 || s > session_max;
            start[j] = st;
            member[j] = st || kind == 1;
        }
        carry_s = apply(shfl64(f, WAVE - 1), carry_s);
        carry_t = (int64_t)shfl64((uint64_t)tj, WAVE - 1);              // (a chunk that is not full is the last)
    }
}

// ---- step 3 -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void sessions_start_kernel(int64_t n, int64_t S0, int64_t U1, int32_t* __restrict__ slen,
                                                             int32_t* __restrict__ suser, int32_t* __restrict__ ukept) {
    const int64_t stride = (int64_t)gridDim.x * TPB;
    for (int64_t i = tid(); i < n; i += stride) {
        if (i < S0) {
            slen[i] = 0;
            suser[i] = -1;
        }
        if (i < U1) ukept[i] = 0;
    }
}

__global__ __launch_bounds__(TPB) void session_len_kernel(const int64_t* __restrict__ keys, const int32_t* __restrict__ start,
                                                          const int32_t* __restrict__ member, const int64_t* __restrict__ scum, int64_t R,
                                                          int64_t S0, int64_t U1, int32_t* __restrict__ slen, int32_t* __restrict__ suser,
                                                          int32_t* __restrict__ status) {
    const int64_t j = tid();
    if (j >= R || !member[j]) return;
    const int64_t s = scum[j] - 1, r = keys[j] >> 32;
    if (s < 0 || s >= S0 || r < 0 || r >= U1) {
        atomicOr(status, MOBGT_CHECKINS_SBADINDEX);
        return;
    }
    atomicAdd(&slen[s], 1);
    if (start[j]) suser[s] = (int32_t)r;
}

__global__ __launch_bounds__(TPB) void user_kept_kernel(const int32_t* __restrict__ slen, const int32_t* __restrict__ suser, int64_t S0,
                                                        int64_t U1, int64_t session_min, int32_t* __restrict__ ukept) {
    const int64_t s = tid();
    if (s >= S0) return;
    const int64_t r = suser[s];
    if (r >= 0 && r < U1 && slen[s] >= session_min) atomicAdd(&ukept[r], 1);
}

// thread i: raw session i and user rank i
__global__ __launch_bounds__(TPB) void select_kernel(const int32_t* __restrict__ slen, const int32_t* __restrict__ suser,
                                                     const int32_t* __restrict__ ukept, int64_t S0, int64_t U1, int64_t session_min,
                                                     int64_t sessions_min, double train_split, int32_t* __restrict__ sfinal,
                                                     int32_t* __restrict__ outlen, int32_t* __restrict__ usurv, int32_t* __restrict__ ukept_s,
                                                     int32_t* __restrict__ split, int32_t* __restrict__ status) {
    const int64_t i = tid();
    if (i < S0) {
        const int64_t r = suser[i];
        const bool fin = r >= 0 && r < U1 && slen[i] >= 1 && slen[i] >= session_min && ukept[r] >= 1 && ukept[r] >= sessions_min;
        sfinal[i] = fin;
        outlen[i] = fin ? slen[i] : 0;
    }
    if (i < U1) {
        const int32_t k = ukept[i];
        const bool surv = k >= 1 && k >= sessions_min;
        const int32_t sp = surv ? (int32_t)floor(train_split * (double)k) : 0;
        usurv[i] = surv;
        ukept_s[i] = surv ? k : 0;
        split[i] = sp;
        if (surv && sp < 1) atomicOr(status, MOBGT_CHECKINS_SZEROSPLIT);
    }
}

__global__ __launch_bounds__(TPB) void emit_flag_kernel(const int32_t* __restrict__ member, const int64_t* __restrict__ scum,
                                                        const int32_t* __restrict__ sfinal, int64_t R, int64_t S0, int32_t* __restrict__ emit) {
    const int64_t j = tid();
    if (j >= R) return;
    const int64_t s = scum[j] - 1;
    emit[j] = member[j] && s >= 0 && s < S0 && sfinal[s];
}

// ---- step 4 -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void first_start_kernel(int64_t n, int64_t M, int64_t P0, int64_t C0, int64_t* __restrict__ kept,
                                                          int32_t* __restrict__ pfirst, int32_t* __restrict__ cfirst) {
    const int64_t stride = (int64_t)gridDim.x * TPB;
    for (int64_t i = tid(); i < n; i += stride) {
        if (i < M) kept[i] = -1;
        if (i < P0) pfirst[i] = INT32_MAX;
        if (i < C0) cfirst[i] = INT32_MAX;
    }
}

__global__ __launch_bounds__(TPB) void first_kernel(const int64_t* __restrict__ keys, const int32_t* __restrict__ emit,
                                                    const int64_t* __restrict__ ocum, int64_t R, int64_t M, const int32_t* __restrict__ poi,
                                                    const int32_t* __restrict__ cat, int64_t N, int64_t P0, int64_t C0,
                                                    int64_t* __restrict__ kept, int32_t* __restrict__ pfirst, int32_t* __restrict__ cfirst,
                                                    int32_t* __restrict__ status) {
    const int64_t j = tid();
    if (j >= R || !emit[j]) return;
    const int64_t o = ocum[j] - 1, i = keys[j] & 0xffffffffll;
    if (o < 0 || o >= M || i >= N) {
        atomicOr(status, MOBGT_CHECKINS_SBADINDEX);
        return;
    }
    const int64_t p = poi[i], c = cat[i];
    if (p < 1 || p > P0 || c < 1 || c > C0) {
        atomicOr(status, MOBGT_CHECKINS_SBADINDEX);
        return;
    }
    kept[o] = i;
    atomicMin(&pfirst[p - 1], (int32_t)o);
    atomicMin(&cfirst[c - 1], (int32_t)o);
}

__global__ __launch_bounds__(TPB) void first_flag_kernel(const int64_t* __restrict__ kept, int64_t M, const int32_t* __restrict__ poi,
                                                         const int32_t* __restrict__ cat, int64_t N, int64_t P0, int64_t C0,
                                                         const int32_t* __restrict__ pfirst, const int32_t* __restrict__ cfirst,
                                                         int32_t* __restrict__ pflag, int32_t* __restrict__ cflag) {
    const int64_t o = tid();
    if (o >= M) return;
    const int64_t i = kept[o];
    int pf = 0, cf = 0;
    if (i >= 0 && i < N) {
        const int64_t p = poi[i], c = cat[i];
        if (p >= 1 && p <= P0) pf = pfirst[p - 1] == o;
        if (c >= 1 && c <= C0) cf = cfirst[c - 1] == o;
    }
    pflag[o] = pf;
    cflag[o] = cf;
}

__global__ __launch_bounds__(TPB) void emit_start_kernel(int64_t n, int64_t M, int64_t P, int64_t n_cat, int64_t S, int64_t U,
                                                         int32_t* __restrict__ seq, int32_t* __restrict__ poi_log, int32_t* __restrict__ cat_log,
                                                         int64_t* __restrict__ offsets, int64_t* __restrict__ users, uint8_t* __restrict__ train,
                                                         int32_t* __restrict__ nn, int32_t* __restrict__ mult, int32_t* __restrict__ user_log) {
    const int64_t stride = (int64_t)gridDim.x * TPB;
    for (int64_t i = tid(); i < n; i += stride) {
        if (i < 3 * M) seq[i] = 0;
        if (i < P) poi_log[i] = -1;
        if (i < n_cat) cat_log[i] = -1;
        if (i <= S) offsets[i] = 0;
        if (i < S) {
            users[i] = -1;
            train[i] = 0;
            nn[i] = 0;
            mult[i] = 0;
        }
        if (i < U) user_log[i] = -1;
    }
}

__global__ __launch_bounds__(TPB) void rows_kernel(const int64_t* __restrict__ kept, const int32_t* __restrict__ pflag,
                                                   const int32_t* __restrict__ cflag, const int64_t* __restrict__ pnum,
                                                   const int64_t* __restrict__ cnum, int64_t M, const int32_t* __restrict__ pfirst,
                                                   const int32_t* __restrict__ cfirst, const int32_t* __restrict__ poi,
                                                   const int32_t* __restrict__ cat, const int64_t* __restrict__ t, int64_t N, int64_t P0,
                                                   int64_t C0, int64_t P, int64_t n_cat, int32_t* __restrict__ seq,
                                                   int32_t* __restrict__ poi_log, int32_t* __restrict__ cat_log, int32_t* __restrict__ status) {
    const int64_t o = tid();
    if (o >= M) return;
    bool ok = false;
    const int64_t i = kept[o];
    if (i >= 0 && i < N) {
        const int64_t p = poi[i];
        if (p >= 1 && p <= P0) {
            const int64_t fo = pfirst[p - 1];                           // the first output check-in of this POI
            if (fo >= 0 && fo < M) {
                const int64_t fi = kept[fo], pid = pnum[fo];
                if (fi >= 0 && fi < N && pid >= 1 && pid <= P) {
                    const int64_t c = cat[fi];                          // its category: the POI's
                    if (c >= 1 && c <= C0) {
                        const int64_t co = cfirst[c - 1];
                        if (co >= 0 && co < M) {
                            const int64_t cid = cnum[co];
                            if (cid >= 1 && cid <= n_cat) {
                                int64_t m = t[i] % 86400;
                                if (m < 0) m += 86400;
                                seq[3 * o] = (int32_t)pid;
                                seq[3 * o + 1] = (int32_t)(m / 1800);
                                seq[3 * o + 2] = (int32_t)cid;
                                ok = true;
                            }
                        }
                    }
                }
            }
        }
        if (pflag[o]) {
            const int64_t pid = pnum[o];
            if (pid >= 1 && pid <= P) poi_log[pid - 1] = (int32_t)i; else ok = false;
        }
        if (cflag[o]) {
            const int64_t cid = cnum[o];
            if (cid >= 1 && cid <= n_cat) cat_log[cid - 1] = (int32_t)i; else ok = false;
        }
    }
    if (!ok) atomicOr(status, MOBGT_CHECKINS_SBADINDEX);
}

// thread i: raw session i and user rank i
__global__ __launch_bounds__(TPB) void pack_kernel(const int32_t* __restrict__ sfinal, const int32_t* __restrict__ suser,
                                                   const int64_t* __restrict__ scum2, const int64_t* __restrict__ lcum, int64_t S0, int64_t S,
                                                   const int64_t* __restrict__ ucum, const int64_t* __restrict__ kcum,
                                                   const int32_t* __restrict__ ukept_s, const int32_t* __restrict__ split, int64_t U1,
                                                   int64_t U, int64_t M, int64_t* __restrict__ offsets, int64_t* __restrict__ users,
                                                   uint8_t* __restrict__ train, int32_t* __restrict__ user_log, int32_t* __restrict__ status) {
    const int64_t i = tid();
    if (i < S0 && sfinal[i]) {
        const int64_t sn = scum2[i] - 1, r = suser[i], end = lcum[i];
        if (sn < 0 || sn >= S || r < 0 || r >= U1 || end < 0 || end > M) {
            atomicOr(status, MOBGT_CHECKINS_SBADINDEX);
        } else {
            offsets[sn + 1] = end;
            users[sn] = ucum[r] - 1;
            train[sn] = sn - (kcum[r] - ukept_s[r]) < split[r];        // the user's first `split` sessions
        }
    }
    if (i < U1 && ukept_s[i] > 0) {
        const int64_t un = ucum[i] - 1;
        if (un >= 0 && un < U) user_log[un] = (int32_t)i; else atomicOr(status, MOBGT_CHECKINS_SBADINDEX);
    }
}

// distinct POIs of the history rows and the largest multiplicity among them: a session has at most 16 rows
__global__ __launch_bounds__(TPB) void distinct_kernel(const int32_t* __restrict__ seq, const int64_t* __restrict__ offsets, int64_t S,
                                                       int64_t M, int32_t* __restrict__ nn, int32_t* __restrict__ mult,
                                                       int32_t* __restrict__ status) {
    const int64_t s = tid();
    if (s >= S) return;
    const int64_t a = offsets[s], b = offsets[s + 1] - 1;               // history rows a .. b - 1
    if (a < 0 || b < a || b >= M || b - a > MOBGT_CHECKINS_MAX_SESSION_MAX + 1) {
        atomicOr(status, MOBGT_CHECKINS_SBADINDEX);
        return;
    }
    int distinct = 0, most = 0;
    for (int64_t x = a; x < b; ++x) {
        const int32_t p = seq[3 * x];
        int same = 0;
        bool seen = false;
        for (int64_t y = a; y < b; ++y) {
            if (seq[3 * y] == p) {
                ++same;
                if (y < x) seen = true;
            }
        }
        if (!seen) ++distinct;
        most = same > most ? same : most;
    }
    nn[s] = distinct;
    mult[s] = most;
}

// null only where the buffer has no element
bool bad_ptr(const void* p, uintptr_t align, int64_t n) {
    return (p == nullptr && n > 0) || (reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0;
}

bool bad_spaces(int64_t N, int64_t U0, int64_t P0, int64_t C0) {
    return N < 0 || N > INT32_MAX || U0 < 1 || U0 > MOBGT_CHECKINS_MAX_U0 || P0 < 1 || P0 > MOBGT_CHECKINS_MAX_P0 || C0 < 1 ||
           C0 > MOBGT_CHECKINS_MAX_C0;
}

int64_t max3(int64_t a, int64_t b, int64_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

}  // namespace

#define LAUNCH(kernel, grid, ...)                                                                   \
    do {                                                                                            \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(TPB), 0, (hipStream_t)stream, __VA_ARGS__);     \
        const hipError_t err_ = hipGetLastError();                                                  \
        if (err_ != hipSuccess) return (int)err_;                                                   \
    } while (0)

extern "C" int mobgt_checkins_abi_version(void) { return MOBGT_CHECKINS_ABI_VERSION; }

extern "C" int mobgt_checkins_count(const void* user, const void* poi, const void* cat, int64_t N, int64_t U0, int64_t P0, int64_t C0,
                                    int64_t trace_min, void* ucnt, void* pcnt, void* ufirst, void* ukey, void* status, void* stream) {
    if (bad_spaces(N, U0, P0, C0) || trace_min < 0) return MOBGT_CHECKINS_EBADDIM;
    if (bad_ptr(user, 4, N) || bad_ptr(poi, 4, N) || bad_ptr(cat, 4, N) || bad_ptr(ucnt, 4, U0) || bad_ptr(pcnt, 4, P0) ||
        bad_ptr(ufirst, 4, U0) || bad_ptr(ukey, 8, U0) || bad_ptr(status, 4, 1))
        return MOBGT_CHECKINS_EALIGN;
    const int64_t n = U0 > P0 ? U0 : P0;
    LAUNCH(count_start_kernel, fill_blocks(n), n, U0, P0, (int32_t*)ucnt, (int32_t*)pcnt, (int32_t*)ufirst, (int32_t*)status);
    if (N > 0)
        LAUNCH(count_kernel, blocks(N), (const int32_t*)user, (const int32_t*)poi, (const int32_t*)cat, N, U0, P0, C0, (int32_t*)ucnt,
               (int32_t*)pcnt, (int32_t*)ufirst, (int32_t*)status);
    LAUNCH(user_key_kernel, blocks(U0), (const int32_t*)ucnt, (const int32_t*)ufirst, U0, trace_min, (int64_t*)ukey);
    return 0;
}

extern "C" int mobgt_checkins_keys(const void* user, const void* poi, const void* cat, int64_t N, int64_t U0, int64_t P0, int64_t C0,
                                   const void* urank, int64_t U1, const void* pcnt, int64_t global_visit, void* keys, void* stream) {
    if (bad_spaces(N, U0, P0, C0) || U1 < 0 || U1 > U0 || global_visit < 0) return MOBGT_CHECKINS_EBADDIM;
    if (bad_ptr(user, 4, N) || bad_ptr(poi, 4, N) || bad_ptr(cat, 4, N) || bad_ptr(urank, 4, U0) || bad_ptr(pcnt, 4, P0) ||
        bad_ptr(keys, 8, N))
        return MOBGT_CHECKINS_EALIGN;
    if (N > 0)
        LAUNCH(keys_kernel, blocks(N), (const int32_t*)user, (const int32_t*)poi, (const int32_t*)cat, N, U0, P0, C0,
               (const int32_t*)urank, U1, (const int32_t*)pcnt, global_visit, (int64_t*)keys);
    return 0;
}

extern "C" int mobgt_checkins_cut(const void* keys, int64_t R, const void* t, int64_t N, int64_t U1, int64_t hour_gap_s, int64_t min_gap_s,
                                  int session_max, void* start, void* member, void* status, void* stream) {
    if (N < 0 || N > INT32_MAX || R < 0 || R > N || U1 < 0 || U1 > INT32_MAX || hour_gap_s < 0 || min_gap_s < 0 || session_max < 1 ||
        session_max > MOBGT_CHECKINS_MAX_SESSION_MAX)
        return MOBGT_CHECKINS_EBADDIM;
    if (bad_ptr(keys, 8, R) || bad_ptr(t, 8, N) || bad_ptr(start, 4, R) || bad_ptr(member, 4, R) || bad_ptr(status, 4, 1))
        return MOBGT_CHECKINS_EALIGN;
    if (R > 0 && U1 > 0)
        LAUNCH(cut_kernel, (unsigned)((U1 + WAVES - 1) / WAVES), (const int64_t*)keys, R, (const int64_t*)t, N, U1, hour_gap_s, min_gap_s,
               session_max, (int32_t*)start, (int32_t*)member, (int32_t*)status);
    return 0;
}

extern "C" int mobgt_checkins_sessions(const void* keys, const void* start, const void* member, const void* scum, int64_t R, int64_t S0,
                                       int64_t U1, int64_t session_min, int64_t sessions_min, double train_split, void* slen,
                                       void* suser, void* ukept, void* sfinal, void* outlen, void* usurv, void* ukept_s, void* split,
                                       void* emit, void* status, void* stream) {
    if (R < 0 || R > INT32_MAX || S0 < 0 || S0 > R || U1 < 0 || U1 > INT32_MAX || session_min < 0 || sessions_min < 0 ||
        !(train_split > 0.0 && train_split <= 1.0))
        return MOBGT_CHECKINS_EBADDIM;
    if (bad_ptr(keys, 8, R) || bad_ptr(start, 4, R) || bad_ptr(member, 4, R) || bad_ptr(scum, 8, R) || bad_ptr(slen, 4, S0) ||
        bad_ptr(suser, 4, S0) || bad_ptr(ukept, 4, U1) || bad_ptr(sfinal, 4, S0) || bad_ptr(outlen, 4, S0) || bad_ptr(usurv, 4, U1) ||
        bad_ptr(ukept_s, 4, U1) || bad_ptr(split, 4, U1) || bad_ptr(emit, 4, R) || bad_ptr(status, 4, 1))
        return MOBGT_CHECKINS_EALIGN;
    const int64_t n = S0 > U1 ? S0 : U1;
    if (n > 0) LAUNCH(sessions_start_kernel, fill_blocks(n), n, S0, U1, (int32_t*)slen, (int32_t*)suser, (int32_t*)ukept);
    if (R > 0)
        LAUNCH(session_len_kernel, blocks(R), (const int64_t*)keys, (const int32_t*)start, (const int32_t*)member, (const int64_t*)scum, R,
               S0, U1, (int32_t*)slen, (int32_t*)suser, (int32_t*)status);
    if (S0 > 0)
        LAUNCH(user_kept_kernel, blocks(S0), (const int32_t*)slen, (const int32_t*)suser, S0, U1, session_min, (int32_t*)ukept);
    if (n > 0)
        LAUNCH(select_kernel, blocks(n), (const int32_t*)slen, (const int32_t*)suser, (const int32_t*)ukept, S0, U1, session_min,
               sessions_min, train_split, (int32_t*)sfinal, (int32_t*)outlen, (int32_t*)usurv, (int32_t*)ukept_s, (int32_t*)split,
               (int32_t*)status);
    if (R > 0)
        LAUNCH(emit_flag_kernel, blocks(R), (const int32_t*)member, (const int64_t*)scum, (const int32_t*)sfinal, R, S0, (int32_t*)emit);
    return 0;
}

extern "C" int mobgt_checkins_first(const void* keys, const void* emit, const void* ocum, int64_t R, int64_t M, const void* poi,
                                    const void* cat, int64_t N, int64_t P0, int64_t C0, void* kept, void* pfirst, void* cfirst,
                                    void* pflag, void* cflag, void* status, void* stream) {
    if (bad_spaces(N, 1, P0, C0) || R < 0 || R > N || M < 0 || M > R) return MOBGT_CHECKINS_EBADDIM;
    if (bad_ptr(keys, 8, R) || bad_ptr(emit, 4, R) || bad_ptr(ocum, 8, R) || bad_ptr(poi, 4, N) || bad_ptr(cat, 4, N) ||
        bad_ptr(kept, 8, M) || bad_ptr(pfirst, 4, P0) || bad_ptr(cfirst, 4, C0) || bad_ptr(pflag, 4, M) || bad_ptr(cflag, 4, M) ||
        bad_ptr(status, 4, 1))
        return MOBGT_CHECKINS_EALIGN;
    const int64_t n = max3(M, P0, C0);
    LAUNCH(first_start_kernel, fill_blocks(n), n, M, P0, C0, (int64_t*)kept, (int32_t*)pfirst, (int32_t*)cfirst);
    if (R > 0)
        LAUNCH(first_kernel, blocks(R), (const int64_t*)keys, (const int32_t*)emit, (const int64_t*)ocum, R, M, (const int32_t*)poi,
               (const int32_t*)cat, N, P0, C0, (int64_t*)kept, (int32_t*)pfirst, (int32_t*)cfirst, (int32_t*)status);
    if (M > 0)
        LAUNCH(first_flag_kernel, blocks(M), (const int64_t*)kept, M, (const int32_t*)poi, (const int32_t*)cat, N, P0, C0,
               (const int32_t*)pfirst, (const int32_t*)cfirst, (int32_t*)pflag, (int32_t*)cflag);
    return 0;
}

extern "C" int mobgt_checkins_emit(const void* kept, const void* pflag, const void* cflag, const void* pnum, const void* cnum, int64_t M,
                                   const void* pfirst, const void* cfirst, const void* poi, const void* cat, const void* t, int64_t N,
                                   int64_t P0, int64_t C0, int64_t P, int64_t n_cat, const void* sfinal, const void* suser,
                                   const void* scum2, const void* lcum, int64_t S0, int64_t S, const void* ucum, const void* kcum,
                                   const void* ukept_s, const void* split, int64_t U1, int64_t U, void* seq, void* poi_log, void* cat_log,
                                   void* offsets, void* users, void* train, void* n, void* mult, void* user_log, void* status,
                                   void* stream) {
    if (bad_spaces(N, 1, P0, C0) || M < 0 || M > N || P < 0 || P > M || n_cat < 0 || n_cat > M || S0 < 0 || S0 > INT32_MAX || S < 0 ||
        S > S0 || U1 < 0 || U1 > INT32_MAX || U < 0 || U > U1)
        return MOBGT_CHECKINS_EBADDIM;
    if (bad_ptr(kept, 8, M) || bad_ptr(pflag, 4, M) || bad_ptr(cflag, 4, M) || bad_ptr(pnum, 8, M) || bad_ptr(cnum, 8, M) ||
        bad_ptr(pfirst, 4, P0) || bad_ptr(cfirst, 4, C0) || bad_ptr(poi, 4, N) || bad_ptr(cat, 4, N) || bad_ptr(t, 8, N) ||
        bad_ptr(sfinal, 4, S0) || bad_ptr(suser, 4, S0) || bad_ptr(scum2, 8, S0) || bad_ptr(lcum, 8, S0) || bad_ptr(ucum, 8, U1) ||
        bad_ptr(kcum, 8, U1) || bad_ptr(ukept_s, 4, U1) || bad_ptr(split, 4, U1) || bad_ptr(seq, 4, M) || bad_ptr(poi_log, 4, P) ||
        bad_ptr(cat_log, 4, n_cat) || bad_ptr(offsets, 8, 1) || bad_ptr(users, 8, S) || bad_ptr(train, 1, S) || bad_ptr(n, 4, S) ||
        bad_ptr(mult, 4, S) || bad_ptr(user_log, 4, U) || bad_ptr(status, 4, 1))
        return MOBGT_CHECKINS_EALIGN;
    const int64_t fill = max3(3 * M, S + 1, U);
    LAUNCH(emit_start_kernel, fill_blocks(fill), fill, M, P, n_cat, S, U, (int32_t*)seq, (int32_t*)poi_log, (int32_t*)cat_log,
           (int64_t*)offsets, (int64_t*)users, (uint8_t*)train, (int32_t*)n, (int32_t*)mult, (int32_t*)user_log);
    if (M > 0)
        LAUNCH(rows_kernel, blocks(M), (const int64_t*)kept, (const int32_t*)pflag, (const int32_t*)cflag, (const int64_t*)pnum,
               (const int64_t*)cnum, M, (const int32_t*)pfirst, (const int32_t*)cfirst, (const int32_t*)poi, (const int32_t*)cat,
               (const int64_t*)t, N, P0, C0, P, n_cat, (int32_t*)seq, (int32_t*)poi_log, (int32_t*)cat_log, (int32_t*)status);
    const int64_t su = S0 > U1 ? S0 : U1;
    if (su > 0)
        LAUNCH(pack_kernel, blocks(su), (const int32_t*)sfinal, (const int32_t*)suser, (const int64_t*)scum2, (const int64_t*)lcum, S0, S,
               (const int64_t*)ucum, (const int64_t*)kcum, (const int32_t*)ukept_s, (const int32_t*)split, U1, U, M, (int64_t*)offsets,
               (int64_t*)users, (uint8_t*)train, (int32_t*)user_log, (int32_t*)status);
    if (S > 0)
        LAUNCH(distinct_kernel, blocks(S), (const int32_t*)seq, (const int64_t*)offsets, S, M, (int32_t*)n, (int32_t*)mult,
               (int32_t*)status);
    return 0;
}
