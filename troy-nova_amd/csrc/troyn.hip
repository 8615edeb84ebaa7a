// troyn.hip -- libtroyn.so: plan management, launch logic and the extern "C" boundary
// declared in include/troyn.h.  gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/troyn.h"
#include "behz_kernels.hpp"
#include "behz2_kernels.hpp"
#include "launch.hpp"
#include "crypto_kernels.hpp"
#include "bgv_kernels.hpp"
#include "bgv_chain_kernels.hpp"
#include "bgv_hoist_kernels.hpp"
#include "ring2k_kernels.hpp"
#include "host_math.hpp"
#include "ntt_kernels.hpp"
#include "ksmac_kernels.hpp"
#include "ksmaci_kernels.hpp"
#include "mulpair_half_kernels.hpp"
#include "poly_kernels.hpp"
#include "hoist_kernels.hpp"
#include "ckks_kernels.hpp"
#include "ckks_tables.hpp"
#include "raise_kernels.hpp"

using namespace troyn;

// ---------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

static int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) return fail((int)e_, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// Small host tables (pointer lists, offsets) for kernels that index them travel through a per-thread ring of pinned slots: the copy is
// then truly asynchronous and the caller's array may go away at once.  (Rounds 1-3 copied from the caller's pageable array and waited for
// the STREAM before returning -- i.e. for every kernel queued before: MatmulHelper's 32 multiply-accumulate calls ran one at a time.)
// A slot is reused after the copy that last read it has completed (its event); tables above the slot size take the old path.
namespace {
struct PinnedSlot { void* host = nullptr; hipEvent_t done = nullptr; };
struct PinnedRing {
    static constexpr size_t SLOTS = 8, BYTES = 256u << 10;
    PinnedSlot slot[SLOTS];
    size_t next = 0;
};   // never destroyed: a host thread may end after the runtime has shut down
}  // namespace
static int upload_host_table(hipStream_t s, void* dev, const void* host, size_t bytes) {
    if (bytes == 0) return TROYN_OK;
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    constexpr int MAX_DEVICES = 16;
    static thread_local PinnedRing* rings[MAX_DEVICES] = {};
    if (bytes > PinnedRing::BYTES || device < 0 || device >= MAX_DEVICES) {
        HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));   // `host` belongs to the caller
        return TROYN_OK;
    }
    if (!rings[device]) rings[device] = new PinnedRing;
    PinnedRing& ring = *rings[device];
    PinnedSlot& sl = ring.slot[ring.next];
    if (!sl.host) {
        // a slot is published only when it is complete (buffer AND event): a failure leaves it empty for the next call to retry
        hipEvent_t ev = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        void* host_buf = nullptr;
        const hipError_t me = hipHostMalloc(&host_buf, PinnedRing::BYTES, hipHostMallocPortable);
        if (me != hipSuccess) { (void)hipEventDestroy(ev); return fail((int)me, std::string("hipHostMalloc: ") + hipGetErrorString(me)); }
        sl.done = ev; sl.host = host_buf;
    } else {
        HIP_TRY(hipEventSynchronize(sl.done));
    }
    ring.next = (ring.next + 1) % PinnedRing::SLOTS;
    std::memcpy(sl.host, host, bytes);
    HIP_TRY(hipMemcpyAsync(dev, sl.host, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(sl.done, s));
    return TROYN_OK;
}

#define LAUNCH_CHECK()                                                                     \
    do {                                                                                   \
        hipError_t e_ = hipGetLastError();                                                 \
        if (e_ != hipSuccess) return fail((int)e_, std::string("kernel launch: ") + hipGetErrorString(e_)); \
    } while (0)

extern "C" const char* troyn_last_error(void) { return g_last_error.c_str(); }
extern "C" int troyn_version(void) { return TROYN_VERSION; }

extern "C" int troyn_get_primes(uint64_t factor, size_t bit_size, size_t count, uint64_t* out) {
    if (!out || factor == 0 || bit_size < 2 || bit_size > 62) return fail(TROYN_E_INVALID, "[get_primes] bad argument");
    try {
        std::vector<u64> v = host::get_primes(factor, bit_size, count);
        for (size_t i = 0; i < count; i++) out[i] = v[i];
    } catch (const std::exception& e) {
        return fail(TROYN_E_MODULUS, e.what());
    }
    return TROYN_OK;
}

extern "C" int troyn_coeff_modulus_create(size_t poly_modulus_degree, const size_t* bit_sizes, size_t n, uint64_t* out) {
    // coeff_modulus.cu:65-108
    if (!bit_sizes || !out) return fail(TROYN_E_INVALID, "[CoeffModulus::create] null argument");
    if (poly_modulus_degree > 131072 || poly_modulus_degree < 2) return fail(TROYN_E_INVALID, "[CoeffModulus::create] Invalid poly_modulus_degree.");
    if (n > 64 || n < 1) return fail(TROYN_E_INVALID, "[CoeffModulus::create] Invalid bit_sizes length.");
    for (size_t i = 0; i < n; i++)
        if (bit_sizes[i] > 60 || bit_sizes[i] < 2) return fail(TROYN_E_INVALID, "[CoeffModulus::create] Invalid max_bit_size.");
    std::vector<size_t> handed(61, 0);
    try {
        for (size_t i = 0; i < n; i++) {
            const size_t s = bit_sizes[i];
            size_t total = 0;
            for (size_t k = 0; k < n; k++) total += (bit_sizes[k] == s);
            std::vector<u64> primes = host::get_primes(2 * (u64)poly_modulus_degree, s, total);
            out[i] = primes[total - 1 - handed[s]++];   // prime_table[size].back(); pop_back()
        }
    } catch (const std::exception& e) {
        return fail(TROYN_E_MODULUS, e.what());
    }
    return TROYN_OK;
}

// ---------------------------------------------------------------------------------------
// in-library kernel timer (measurement hook, include/troyn.h): hipEvent pairs recorded on the launch stream
// around one named launch, so that a caller can time that kernel inside its own timed region
// ---------------------------------------------------------------------------------------
namespace {
// events belong to the device that was current when they were created: the pool and the recorded spans are kept per device, so one
// host thread that alternates between devices (select_device) never records a pair on a foreign stream
struct TimerSpan { hipEvent_t e0, e1; int device; };
struct KernelTimer {
    std::atomic<bool> enabled[TROYN_TIMER_REGIONS];
    std::vector<TimerSpan> spans[TROYN_TIMER_REGIONS];   // recorded, not yet read
    std::vector<TimerSpan> free_pairs;                   // reusable pairs of any device
    std::mutex mu;
    KernelTimer() { for (auto& e : enabled) e.store(false); }
};
KernelTimer g_ktimer;

struct TimerScope {
    int region; hipStream_t s; TimerSpan sp{nullptr, nullptr, -1};
    TimerScope(int region_, hipStream_t s_) : region(region_), s(s_) {
        if (!g_ktimer.enabled[region].load(std::memory_order_relaxed)) return;
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess) return;
        {
            std::lock_guard<std::mutex> g(g_ktimer.mu);
            for (size_t i = 0; i < g_ktimer.free_pairs.size(); i++)
                if (g_ktimer.free_pairs[i].device == dev) { sp = g_ktimer.free_pairs[i]; g_ktimer.free_pairs.erase(g_ktimer.free_pairs.begin() + i); break; }
        }
        if (!sp.e0) {
            sp.device = dev;
            if (hipEventCreate(&sp.e0) != hipSuccess) { sp.e0 = nullptr; return; }
            if (hipEventCreate(&sp.e1) != hipSuccess) { (void)hipEventDestroy(sp.e0); sp.e0 = sp.e1 = nullptr; return; }
        }
        if (hipEventRecord(sp.e0, s) != hipSuccess) { release(); }
    }
    void release() {
        std::lock_guard<std::mutex> g(g_ktimer.mu);
        g_ktimer.free_pairs.push_back(sp);
        sp.e0 = sp.e1 = nullptr;
    }
    ~TimerScope() {
        if (!sp.e0) return;
        if (hipEventRecord(sp.e1, s) != hipSuccess) { release(); return; }
        std::lock_guard<std::mutex> g(g_ktimer.mu);
        g_ktimer.spans[region].push_back(sp);
    }
};
}  // namespace

extern "C" int troyn_kernel_timer_enable(int region, int on) {
    if (region < 0 || region >= TROYN_TIMER_REGIONS) return fail(TROYN_E_INVALID, "[troyn_kernel_timer_enable] unknown region");
    g_ktimer.enabled[region].store(on != 0);
    return TROYN_OK;
}

extern "C" int troyn_kernel_timer_read(int region, double* total_ms, uint64_t* launches) {
    if (region < 0 || region >= TROYN_TIMER_REGIONS || !total_ms || !launches) return fail(TROYN_E_INVALID, "[troyn_kernel_timer_read] bad argument");
    std::vector<TimerSpan> spans;
    { std::lock_guard<std::mutex> g(g_ktimer.mu); spans.swap(g_ktimer.spans[region]); }
    double total = 0.0;
    hipError_t err = hipSuccess;
    int cur = -1;
    (void)hipGetDevice(&cur);
    for (auto& sp : spans) {
        if (err != hipSuccess) break;
        if (sp.device != cur) { if ((err = hipSetDevice(sp.device)) != hipSuccess) break; }
        float ms = 0.f;
        if ((err = hipEventSynchronize(sp.e1)) == hipSuccess && (err = hipEventElapsedTime(&ms, sp.e0, sp.e1)) == hipSuccess) total += ms;
        if (sp.device != cur) (void)hipSetDevice(cur);
    }
    {   // the pairs go back to the pool whatever happened: nothing leaks, no sample is half-read
        std::lock_guard<std::mutex> g(g_ktimer.mu);
        for (auto& sp : spans) g_ktimer.free_pairs.push_back(sp);
    }
    if (err != hipSuccess) return fail((int)err, std::string("[troyn_kernel_timer_read] ") + hipGetErrorString(err));
    *total_ms = total; *launches = spans.size();
    return TROYN_OK;
}

// ---------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------
// A/B switches.  Rounds 1-4 read them from the environment on EVERY library call (getenv is not safe against a concurrent setenv, and
// host threads of the C++ mirror run the library concurrently); since round 5 they are read ONCE, when a plan is created, into the plan
// (troyn_plan_create), and changed per plan with troyn_plan_set_option(plan, "TROYN_...", "value") -- no environment access on any call path.
struct TroynOptions {
    bool ntt_u64 = false;            // TROYN_NTT_ARITH=u64: integer butterflies (and the integer inner product) for every modulus
    int ntt_split = -1;              // TROYN_NTT_SPLIT=0|1: launches over limbs of both classes as one integer launch / always split by class
    bool tensor_split = false;       // TROYN_BFV_TENSOR=split: separate transform and dyadic launches in the BFV multiply
    bool tensor_fused = false;       // TROYN_BFV_TENSOR=fused: tensor_core_kernel also for launches of a few ciphertexts (whole-limb sizes, see troyn_bfv_multiply)
    int ks_order = -1;               // TROYN_KS_ORDER=plain|item|row|band (0..3): workgroup order of the inner product kernels
    int ks_split = -1;               // TROYN_KS_SPLIT=0|1: digit-parallel inner product off / forced on
    bool ks_tail_split = false;      // TROYN_KS_TAIL=split: coefficient-form tail as separate launches
    bool ks_mac_split = false;       // TROYN_KS_MAC=split: decomposition NTT and inner product in two launches (the path of N < 1024 / N > 32768)
    bool ks_mac_fused = false;       // TROYN_KS_MAC=fused: the one-launch inner product also for small launches of chains with moduli >= 2^50 (see ks_small_mixed)
    bool ks_diag_loop = false;       // TROYN_KS_DIAG=loop: diagonal digit as an iteration of ksmac2's digit loop
    int ks_rows = 0;                 // TROYN_KS_ROWS=<r>: rows co-scheduled per XCD by the whole-limb inner product of N < 8192
    bool ks_mac_shoup_off = false;   // TROYN_KS_MAC_SHOUP=0: Barrett-128 terms in that kernel's integer form
    bool mrr_mixed_off = false;      // TROYN_MRR_MIXED=0: chains with moduli >= 2^50 compose the three calls inside the fused entry
    bool mrr_small_off = false;      // TROYN_MRR_SMALL=0: single objects at N = 16384 keep the six-launch tail of the fused chain
    bool mrr_small_serial = false;   // TROYN_MRR_SMALL=serial: one thread per quartet loops over the output limbs (no recomputation of the inverse tails)
    bool mrr_calls = false;          // TROYN_MRR=calls: the fused entry composes the three public calls
    int mrr_chunk = 0, mrr_streams = 2;   // TROYN_MRR_CHUNK=<items>, TROYN_MRR_STREAMS=<1..4>
    bool behz_v1 = false;            // TROYN_BEHZ=v1: first-generation conversion kernels (they stay the path of L > 16 and N < 1024)
    bool behz_base_ref = false;      // TROYN_BEHZ_BASE=ref: the reference's auxiliary base of 61-bit primes also when every q_i is below 2^50 (read by
                                     // troyn_behz_create; default since round 5: a base of primes below 2^50 there, "small" = that default)
    bool behz_lift_split = false;    // TROYN_BEHZ_LIFT=split: N = 32768 lifts an operand in three launches (first pass, lift, first pass) instead of one
    int plain_mac = 0;               // TROYN_PLAIN_MAC=v1|single|dual|quad (1..4): grouping of the ct x pt multiply-accumulate
    int ntt_half = -1;               // TROYN_NTT_HALF=<mask>
    bool ntt_overlap_off = false;    // TROYN_NTT_OVERLAP=0: the per-class launches of a chain with wide moduli run one after the other on the caller's stream
    bool ntt_small_two_pass_off = false;   // TROYN_NTT_SMALL_TWO_PASS=0
    int tensor_wgs = 8;              // TROYN_TENSOR_WGS=8|3|2
    bool mulpair_half_off = false;   // TROYN_MULPAIR_HALF=0: step (1) of the fused chain keeps the whole-limb kernel at N = 16384 (mulpair_half_kernels.hpp)
};
static const char* const TROYN_OPTION_NAMES[] = {"TROYN_NTT_ARITH", "TROYN_NTT_SPLIT", "TROYN_BFV_TENSOR", "TROYN_KS_ORDER", "TROYN_KS_SPLIT", "TROYN_KS_TAIL", "TROYN_KS_MAC",
    "TROYN_KS_DIAG", "TROYN_KS_ROWS", "TROYN_KS_MAC_SHOUP", "TROYN_MRR_MIXED", "TROYN_MRR_SMALL", "TROYN_MRR", "TROYN_MRR_CHUNK", "TROYN_MRR_STREAMS", "TROYN_BEHZ", "TROYN_BEHZ_BASE", "TROYN_BEHZ_LIFT",
    "TROYN_PLAIN_MAC", "TROYN_NTT_HALF", "TROYN_NTT_SMALL_TWO_PASS", "TROYN_TENSOR_WGS", "TROYN_NTT_OVERLAP", "TROYN_MULPAIR_HALF"};
// value == nullptr or "": the option's default.  Returns 1 = applied, 0 = unknown name, -1 = a value this option does not have (nothing is changed:
// a misspelt value must not silently select a variant -- TROYN_TENSOR_WGS=foo used to parse as 0 and pick the two-workgroup kernel).
static int option_apply(TroynOptions& o, const char* name, const char* value) {
    const TroynOptions d;
    const std::string n = name ? name : "", v = value ? value : "";
    bool bad = false;
    // one of the listed words (index), or the default for ""; anything else is invalid
    auto word = [&](std::initializer_list<const char*> words, int dflt) {
        if (v.empty()) return dflt;
        int i = 0;
        for (const char* w : words) { if (v == w) return i; i++; }
        bad = true;
        return dflt;
    };
    auto num = [&](long lo, long hi, int dflt) {
        if (v.empty()) return dflt;
        char* end = nullptr;
        const long x = strtol(v.c_str(), &end, 0);
        if (end == v.c_str() || *end || x < lo || x > hi) { bad = true; return dflt; }
        return (int)x;
    };
    TroynOptions t = o;
    if (n == "TROYN_NTT_ARITH") t.ntt_u64 = word({"auto", "u64"}, 0) == 1;
    else if (n == "TROYN_NTT_SPLIT") t.ntt_split = num(0, 1, d.ntt_split);
    else if (n == "TROYN_BFV_TENSOR") { const int w = word({"auto", "split", "fused"}, 0); t.tensor_split = w == 1; t.tensor_fused = w == 2; }
    else if (n == "TROYN_KS_ORDER") t.ks_order = word({"plain", "item", "row", "band"}, d.ks_order);
    else if (n == "TROYN_KS_SPLIT") t.ks_split = num(0, 1, d.ks_split);
    else if (n == "TROYN_KS_TAIL") t.ks_tail_split = word({"fused", "split"}, 0) == 1;
    else if (n == "TROYN_KS_MAC") { const int w = word({"auto", "split", "fused"}, 0); t.ks_mac_split = w == 1; t.ks_mac_fused = w == 2; }
    else if (n == "TROYN_KS_DIAG") t.ks_diag_loop = word({"epilogue", "loop"}, 0) == 1;
    else if (n == "TROYN_KS_ROWS") t.ks_rows = num(0, 64, d.ks_rows);
    else if (n == "TROYN_KS_MAC_SHOUP") t.ks_mac_shoup_off = num(0, 1, 1) == 0;
    else if (n == "TROYN_MRR_MIXED") t.mrr_mixed_off = num(0, 1, 1) == 0;
    else if (n == "TROYN_MRR_SMALL") { const int w = word({"1", "0", "serial"}, 0); t.mrr_small_off = w == 1; t.mrr_small_serial = w == 2; }
    else if (n == "TROYN_MRR") t.mrr_calls = word({"fused", "calls"}, 0) == 1;
    else if (n == "TROYN_MRR_CHUNK") t.mrr_chunk = num(0, 1 << 20, d.mrr_chunk);
    else if (n == "TROYN_MRR_STREAMS") t.mrr_streams = num(1, 4, d.mrr_streams);
    else if (n == "TROYN_BEHZ") t.behz_v1 = word({"v2", "v1"}, 0) == 1;
    else if (n == "TROYN_BEHZ_BASE") t.behz_base_ref = word({"small", "ref"}, 0) == 1;
    else if (n == "TROYN_BEHZ_LIFT") t.behz_lift_split = word({"fused", "split"}, 0) == 1;
    else if (n == "TROYN_PLAIN_MAC") t.plain_mac = word({"auto", "v1", "single", "dual", "quad"}, 0);
    else if (n == "TROYN_NTT_HALF") t.ntt_half = num(0, 0xffff, d.ntt_half);
    else if (n == "TROYN_NTT_SMALL_TWO_PASS") t.ntt_small_two_pass_off = num(0, 1, 1) == 0;
    else if (n == "TROYN_NTT_OVERLAP") t.ntt_overlap_off = num(0, 1, 1) == 0;
    else if (n == "TROYN_MULPAIR_HALF") t.mulpair_half_off = num(0, 1, 1) == 0;
    else if (n == "TROYN_TENSOR_WGS") { t.tensor_wgs = num(2, 8, d.tensor_wgs); if (t.tensor_wgs != 8 && t.tensor_wgs != 3 && t.tensor_wgs != 2) bad = true; }
    else return 0;
    if (bad) return -1;
    o = t;
    return 1;
}
// the ONLY place the library reads its switches from the environment (troyn_plan_create); a value an option does not have fails the creation
static int options_from_environment(TroynOptions& o) {
    for (const char* name : TROYN_OPTION_NAMES)
        if (const char* e = getenv(name))
            if (option_apply(o, name, e) < 0) return fail(TROYN_E_INVALID, std::string("[troyn_plan_create] environment: ") + name + "=" + e + " is not a value of this option");
    return TROYN_OK;
}

struct troyn_plan {
    int device = 0;
    TroynOptions opt;
    std::atomic<uint64_t> opt_gen{0};     // bumped by troyn_plan_set_option: handles that own a second plan (troyn_behz: the auxiliary base) re-read `opt` when it moved
    unsigned log_n = 0, n = 0, K = 0;
    std::vector<u64> moduli;
    std::vector<host::NttTable> tables;   // host copies (KAT hooks, BEHZ construction)
    DevModulus* d_mods = nullptr;         // [K]
    ulonglong2* d_fwd = nullptr;          // [K][N]
    ulonglong2* d_inv = nullptr;          // [K][N]
    double* d_fwd_f64 = nullptr;          // [K][N] w as double for moduli < 2^50 (zeros otherwise)
    double* d_inv_f64 = nullptr;          // [K][N]
    std::vector<char> small_modulus;      // [K] 1 iff q < 2^50 (FP64 fast path usable)
    ulonglong2* d_inv_last = nullptr;     // [(K+1)][K]: row L holds q_{L-1}^-1 mod q_i, i < L-1
    // ksmac2_kernel (N = 8192 / 16384, moduli < 2^50): the forward twiddles in the order its register rounds read them
    double* d_fwd_r1 = nullptr;           // [K][N/1024][32]
    double* d_fwd_r2 = nullptr;           // [K][N], lane-interleaved (ksm_perm)
    // ksmaci_kernel (same sizes, any modulus): the same two copies as (operand, quotient) pairs
    ulonglong2* d_fwd_r1i = nullptr;      // [K][N/1024][32]
    ulonglong2* d_fwd_r2i = nullptr;      // [K][N], lane-interleaved (ksm_perm)
    // mulpair_half_kernel (N = 16384, moduli < 2^50): the inverse twiddles in the order ITS register rounds read them
    double* d_inv_r1 = nullptr;           // [K][N/1024][32]
    double* d_inv_r2 = nullptr;           // [K][N], lane-interleaved (ksm_perm)
};

// One host thread may drive several devices (the reference calls utils::set_device before every launch, fgk/ntt_grouped.cu:286):
// every entry point that takes a handle makes that handle's device current first.
static inline void select_device_index(int device) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != device) (void)hipSetDevice(device);
}
static inline void select_device(const troyn_plan* p) { if (p) select_device_index(p->device); }
template <typename H> static inline void select_device(const H* h) { if (h && h->plan) select_device_index(h->plan->device); }


static DevModulus make_dev_modulus(u64 q, unsigned log_n, bool with_inv_n) {
    DevModulus m;
    std::memset(&m, 0, sizeof(m));
    m.q = q;
    host::BarrettRatio r = host::barrett_ratio(q);
    m.ratio_lo = r.lo; m.ratio_hi = r.hi;
    if (with_inv_n) {
        u64 ninv = 0;
        if (host::invmod(((u64)1 << log_n) % q, q, ninv)) {
            host::Shoup s = host::shoup(ninv, q);
            m.inv_n_op = s.operand; m.inv_n_quo = s.quotient;
            if (q < F64_MODULUS_LIMIT) { m.inv_n_d = (double)ninv; m.inv_n_pd = (double)ninv * (1.0 / (double)q); }
        }
    }
    if (q < F64_MODULUS_LIMIT) { m.pd = (double)q; m.inv_pd = 1.0 / (double)q; }
    return m;
}

static inline ulonglong2 shoup_pair(u64 w, u64 m) {
    const host::Shoup s = host::shoup(w % m, m);
    return make_ulonglong2(s.operand, s.quotient);
}

static auto element_of(const std::vector<u64>& v) { return [&v](size_t i) { return v[i]; }; }

// (q/q_i)^-1 mod q_i for every prime of a base (RNSBase::initialize); 1 for a base of one prime
static int inv_punctured(const std::vector<u64>& q, std::vector<u64>& out) {
    out.assign(q.size(), 1);
    for (size_t i = 0; q.size() > 1 && i < q.size(); i++)
        if (!host::invmod(host::product_mod(q, i, q[i]) % q[i], q[i], out[i])) return fail(TROYN_E_MODULUS, "[RNSBase::initialize] RNSBase product is not invertible.");
    return TROYN_OK;
}

template <typename T>
static int upload_vector(T** dev, const std::vector<T>& v) {
    HIP_TRY(hipMalloc(dev, v.size() * sizeof(T)));
    HIP_TRY(hipMemcpy(*dev, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return TROYN_OK;
}

// The constant tables of one handle (troyn_behz, troyn_bgv, troyn_ring2k): rows are appended on the host and uploaded as one allocation.
// An append returns the offset (in words) of its row; bind() names the pointer that upload() sets to that row.  A row of 16-byte elements starts on 16 bytes.
struct ConstBlob {
    std::vector<u64> host;
    std::vector<std::function<void(const u64*)>> bound;
    std::vector<u64>& aligned() { if (host.size() & 1) host.push_back(0); return host; }
    template <typename F>
    size_t words(size_t count, F f) {
        const size_t off = host.size();
        for (size_t i = 0; i < count; i++) host.push_back(f(i));
        return off;
    }
    // (operand, quotient) of f(i) mod modulus_of(i)
    template <typename F, typename M>
    size_t shoup(size_t count, F f, M modulus_of) {
        const size_t off = aligned().size();
        for (size_t i = 0; i < count; i++) { const ulonglong2 s = shoup_pair(f(i), modulus_of(i)); host.push_back(s.x); host.push_back(s.y); }
        return off;
    }
    template <typename T> static const T* at(const u64* dev, size_t off) { return reinterpret_cast<const T*>(dev + off); }
    template <typename T> void bind(const T** field, size_t off) { bound.push_back([=](const u64* dev) { *field = at<T>(dev, off); }); }
    int upload(int device, u64** dev) const {
        HIP_TRY(hipSetDevice(device));
        if (int rc = upload_vector(dev, host)) return rc;
        for (const auto& set : bound) set(*dev);
        return TROYN_OK;
    }
};

// One value per twiddle of every modulus, [K][N]: conv(i, w) of table entry w of modulus i
template <typename T, typename Conv>
static std::vector<T> twiddle_rows(const troyn_plan* p, bool inverse, Conv conv) {
    std::vector<T> rows;
    rows.reserve((size_t)p->K * p->n);
    for (size_t i = 0; i < p->K; i++)
        for (const host::Shoup& w : inverse ? p->tables[i].inv : p->tables[i].fwd) rows.push_back(conv(i, w));
    return rows;
}

// Round vectors of ksmac2_kernel / ksmaci_kernel, the forward twiddles in the order their register rounds read them: slot s = (1 << lvl) + g of the
// thread (round 2) / of the index bits above bit 9 (round 1) holds the twiddle of butterfly group g of the round's layer lvl (ksmac_kernels.hpp).
// r1: [K][N/1024][32], r2: [K][N] lane-interleaved (ksm_perm); conv(i, w) as in twiddle_rows.
template <typename T, typename Conv>
static void round_vectors(const troyn_plan* p, Conv conv, std::vector<T>& r1, std::vector<T>& r2) {
    const size_t K = p->K, n = p->n, r1n = (n >> 10) * 32;
    r1.assign(K * r1n, conv(0, host::Shoup{0, 0}));
    r2.assign(K * n, conv(0, host::Shoup{0, 0}));
    for (size_t i = 0; i < K; i++) {
        const auto& fw = p->tables[i].fwd;
        for (unsigned s = 1; s < 32; s++) {
            unsigned lvl = 0;
            while ((2u << lvl) <= s) lvl++;
            const unsigned g = s - (1u << lvl);
            for (size_t th = 0; th < (n >> 10); th++) r1[i * r1n + th * 32 + s] = conv(i, fw[(((n >> 10) + th) << lvl) + g]);
            for (size_t T_ = 0; T_ < (n >> 5); T_++) r2[i * n + ksm_perm((unsigned)(T_ * 32 + s))] = conv(i, fw[(((n >> 5) + T_) << lvl) + g]);
        }
    }
}

// The same two copies of the INVERSE twiddles for mulpair_half_kernel, whose rounds walk ksmac2's backwards: round A keeps tile bits [0, 5) in
// registers (r2: per thread T = index >> 5), round B bits [5, 10) (r1: per value th of the index bits above bit 9).  Slot (1 << lvl) + g holds the
// twiddle of butterfly group g of register bit 4 - lvl: Gentleman-Sande layer of index bit `bit` = forward-numbered layer l = log_n - 1 - bit,
// table entry n - (2 << l) + 1 + (index >> (bit + 1))  (ntt_pass_body).
template <typename T, typename Conv>
static void inverse_round_vectors(const troyn_plan* p, Conv conv, std::vector<T>& r1, std::vector<T>& r2) {
    const size_t K = p->K, n = p->n, r1n = (n >> 10) * 32;
    r1.assign(K * r1n, conv(0, host::Shoup{0, 0}));
    r2.assign(K * n, conv(0, host::Shoup{0, 0}));
    for (size_t i = 0; i < K; i++) {
        const auto& iv = p->tables[i].inv;
        for (unsigned s = 1; s < 32; s++) {
            unsigned lvl = 0;
            while ((2u << lvl) <= s) lvl++;
            const unsigned g = s - (1u << lvl);
            for (size_t th = 0; th < (n >> 10); th++) r1[i * r1n + th * 32 + s] = conv(i, iv[n - ((n >> 9) << lvl) + 1 + (th << lvl) + g]);
            for (size_t T_ = 0; T_ < (n >> 5); T_++) r2[i * n + ksm_perm((unsigned)(T_ * 32 + s))] = conv(i, iv[n - ((n >> 4) << lvl) + 1 + (T_ << lvl) + g]);
        }
    }
}

static int plan_upload(troyn_plan* p) {
    const size_t K = p->K, n = p->n;
    std::vector<DevModulus> mods(K);
    p->small_modulus.assign(K, 0);
    for (size_t i = 0; i < K; i++) {
        mods[i] = make_dev_modulus(p->moduli[i], p->log_n, true);
        mods[i].inv_n_op = p->tables[i].inv_degree.operand;
        mods[i].inv_n_quo = p->tables[i].inv_degree.quotient;
        p->small_modulus[i] = p->moduli[i] < F64_MODULUS_LIMIT;
        if (p->small_modulus[i] && n >= 2) {
            // the final Gentleman-Sande layer has one twiddle (table index N-1); N^-1 is folded into it
            const u64 nw = host::mulmod(p->tables[i].inv[n - 1].operand, p->tables[i].inv_degree.operand, p->moduli[i]);
            mods[i].inv_n_w_d = (double)nw;
            mods[i].inv_n_w_pd = (double)nw * (1.0 / (double)p->moduli[i]);
        }
    }
    std::vector<ulonglong2> inv_last((K + 1) * K, make_ulonglong2(0, 0));
    for (size_t L = 2; L <= K; L++)
        for (size_t i = 0; i + 1 < L; i++) {
            u64 inv = 0;
            if (!host::invmod(p->moduli[L - 1] % p->moduli[i], p->moduli[i], inv))
                return fail(TROYN_E_MODULUS, "[troyn_plan_create] Unable to invert q[last] mod q[i].");
            inv_last[L * K + i] = shoup_pair(inv, p->moduli[i]);
        }
    static_assert(sizeof(host::Shoup) == sizeof(ulonglong2), "Shoup layout");
    // the integer kernels read (operand, quotient); the FP64 ones w as an exact double, for the moduli below 2^50 (zeros otherwise)
    auto pair = [](size_t, const host::Shoup& w) { return make_ulonglong2(w.operand, w.quotient); };
    auto f64 = [&](size_t i, const host::Shoup& w) { return p->small_modulus[i] ? (double)w.operand : 0.0; };
    int rc;
    if ((rc = upload_vector(&p->d_mods, mods))) return rc;
    if ((rc = upload_vector(&p->d_fwd, twiddle_rows<ulonglong2>(p, false, pair)))) return rc;
    if ((rc = upload_vector(&p->d_inv, twiddle_rows<ulonglong2>(p, true, pair)))) return rc;
    if ((rc = upload_vector(&p->d_inv_last, inv_last))) return rc;
    if ((rc = upload_vector(&p->d_fwd_f64, twiddle_rows<double>(p, false, f64)))) return rc;
    if ((rc = upload_vector(&p->d_inv_f64, twiddle_rows<double>(p, true, f64)))) return rc;
    if (p->log_n >= 13 && p->log_n <= 15) {
        std::vector<double> r1, r2;
        round_vectors(p, f64, r1, r2);
        if ((rc = upload_vector(&p->d_fwd_r1, r1)) || (rc = upload_vector(&p->d_fwd_r2, r2))) return rc;
        // the integer copies (ksmaci_kernel), every modulus: a chain of narrow moduli can be forced onto the integer kernels (TROYN_NTT_ARITH=u64)
        std::vector<ulonglong2> r1i, r2i;
        round_vectors(p, pair, r1i, r2i);
        if ((rc = upload_vector(&p->d_fwd_r1i, r1i)) || (rc = upload_vector(&p->d_fwd_r2i, r2i))) return rc;
    }
    if (p->log_n == 14) {
        std::vector<double> r1, r2;
        inverse_round_vectors(p, f64, r1, r2);
        if ((rc = upload_vector(&p->d_inv_r1, r1)) || (rc = upload_vector(&p->d_inv_r2, r2))) return rc;
    }
    return TROYN_OK;
}

static void plan_free(troyn_plan* p) {
    if (!p) return;
    if (p->d_mods) (void)hipFree(p->d_mods);
    if (p->d_fwd) (void)hipFree(p->d_fwd);
    if (p->d_inv) (void)hipFree(p->d_inv);
    if (p->d_inv_last) (void)hipFree(p->d_inv_last);
    if (p->d_fwd_f64) (void)hipFree(p->d_fwd_f64);
    if (p->d_inv_f64) (void)hipFree(p->d_inv_f64);
    if (p->d_fwd_r1) (void)hipFree(p->d_fwd_r1);
    if (p->d_fwd_r2) (void)hipFree(p->d_fwd_r2);
    if (p->d_fwd_r1i) (void)hipFree(p->d_fwd_r1i);
    if (p->d_fwd_r2i) (void)hipFree(p->d_fwd_r2i);
    if (p->d_inv_r1) (void)hipFree(p->d_inv_r1);
    if (p->d_inv_r2) (void)hipFree(p->d_inv_r2);
    delete p;
}

extern "C" int troyn_plan_create(troyn_plan** plan, int device, uint32_t log_n, uint32_t n_moduli,
                                 const uint64_t* moduli, const uint64_t* roots) {
    if (!plan || !moduli) return fail(TROYN_E_INVALID, "[troyn_plan_create] null argument");
    *plan = nullptr;
    if (log_n < 1 || log_n > 17) return fail(TROYN_E_INVALID, "[troyn_plan_create] Invalid poly_modulus_degree.");
    if (n_moduli < 1 || n_moduli > 64) return fail(TROYN_E_INVALID, "[troyn_plan_create] Invalid coeff modulus count.");
    std::unique_ptr<troyn_plan, void (*)(troyn_plan*)> p(new troyn_plan, plan_free);
    p->device = device; p->log_n = log_n; p->n = 1u << log_n; p->K = n_moduli;
    { const int orc = options_from_environment(p->opt); if (orc != TROYN_OK) return orc; }
    p->moduli.assign(moduli, moduli + n_moduli);
    for (uint32_t i = 0; i < n_moduli; i++) {
        u64 q = moduli[i];
        if ((q >> 61) != 0 || q < 2) return fail(TROYN_E_MODULUS, "[Modulus::set_value] Value can be at most 61-bit and cannot be 1.");
        for (uint32_t j = 0; j < i; j++)
            if (moduli[j] == q) return fail(TROYN_E_MODULUS, "[troyn_plan_create] coeff_modulus must be pairwise coprime.");
        try {
            p->tables.push_back(host::make_ntt_table(log_n, q, roots ? roots[i] : 0));
        } catch (const std::exception& e) {
            return fail(TROYN_E_MODULUS, e.what());
        }
    }
    HIP_TRY(hipSetDevice(device));
    int rc = plan_upload(p.get());
    if (rc != TROYN_OK) return rc;
    *plan = p.release();
    return TROYN_OK;
}

extern "C" int troyn_plan_destroy(troyn_plan* plan) {
    plan_free(plan);
    return TROYN_OK;
}

extern "C" int troyn_plan_set_option(troyn_plan* plan, const char* name, const char* value) {
    if (!plan || !name) return fail(TROYN_E_INVALID, "[troyn_plan_set_option] null argument");
    // (a handle created from this plan -- troyn_behz, troyn_bgv, ... -- reads the plan's options at call time; TROYN_BEHZ_BASE is read by troyn_behz_create)
    const int rc = option_apply(plan->opt, name, value);
    if (rc == 0) return fail(TROYN_E_INVALID, std::string("[troyn_plan_set_option] unknown option ") + name);
    if (rc < 0) return fail(TROYN_E_INVALID, std::string("[troyn_plan_set_option] ") + name + "=" + value + " is not a value of this option");
    plan->opt_gen.fetch_add(1, std::memory_order_release);
    return TROYN_OK;
}

extern "C" uint32_t troyn_plan_log_n(const troyn_plan* plan) { return plan ? plan->log_n : 0; }
extern "C" uint32_t troyn_plan_n_moduli(const troyn_plan* plan) { return plan ? plan->K : 0; }

extern "C" int troyn_plan_get_root(const troyn_plan* plan, uint32_t mi, uint64_t* root) {
    select_device(plan);
    if (!plan || !root || mi >= plan->K) return fail(TROYN_E_INVALID, "[troyn_plan_get_root] bad argument");
    *root = plan->tables[mi].root;
    return TROYN_OK;
}

extern "C" int troyn_plan_get_root_powers(const troyn_plan* plan, uint32_t mi, int inverse, uint64_t* out) {
    select_device(plan);
    if (!plan || !out || mi >= plan->K) return fail(TROYN_E_INVALID, "[troyn_plan_get_root_powers] bad argument");
    const auto& v = inverse ? plan->tables[mi].inv : plan->tables[mi].fwd;
    for (size_t i = 0; i < v.size(); i++) { out[2 * i] = v[i].operand; out[2 * i + 1] = v[i].quotient; }
    return TROYN_OK;
}

// ---------------------------------------------------------------------------------------
// NTT launch
// ---------------------------------------------------------------------------------------
// (the A/B switches live in the plan: TroynOptions above)
static inline bool force_integer_ntt(const troyn_plan* p) { return p->opt.ntt_u64; }
static inline LaunchCtx launch_ctx(const troyn_plan* p, hipStream_t s) { return LaunchCtx{s, p->opt.ntt_half, p->opt.ntt_small_two_pass_off, p->opt.tensor_wgs}; }

// Launches over limbs of BOTH arithmetic classes are issued once per run of limbs of one class (limbs are independent).  The integer runs are bound
// by vector-ALU issue, the FP64 runs of the memory-side kernels by memory latency / bandwidth, so two such runs in flight fill each other's idle
// resource: every other run goes to a side stream (one per host thread and device, non-blocking), forked from the caller's stream by an event and
// joined back to it before the call returns -- the caller still sees one stream order.  Only for launches large enough to fill the chip on their own
// (a handful of workgroups gains nothing from a second queue and pays two event waits).  TROYN_NTT_OVERLAP=0: one run after the other.
namespace {
struct SideStream { hipStream_t s = nullptr; hipEvent_t fork = nullptr, join = nullptr; };
// one side stream per host thread and device, created on first use and destroyed when the host thread ends (the reference tool's -c N mode spawns such
// threads per run: round 5 leaked a stream and two events per thread).  Fixed slots: a pointer handed out stays valid while other devices are added.
struct SideStreams {
    static constexpr int MAX_DEVICES = 16;
    SideStream slot[MAX_DEVICES];
    ~SideStreams() {
        for (SideStream& x : slot) {
            if (!x.s) continue;
            (void)hipEventDestroy(x.fork); (void)hipEventDestroy(x.join); (void)hipStreamDestroy(x.s);
            (void)hipGetLastError();       // (a thread that ends while the runtime shuts down: nothing left to release)
        }
    }
};
SideStream* side_stream(int device) {
    static thread_local SideStreams pool;
    if (device < 0 || device >= SideStreams::MAX_DEVICES) return nullptr;
    SideStream& x = pool.slot[device];
    if (x.s) return &x;
    hipStream_t st = nullptr; hipEvent_t f = nullptr, j = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (hipEventCreateWithFlags(&f, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&j, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        if (f) (void)hipEventDestroy(f);
        (void)hipStreamDestroy(st);
        return nullptr;
    }
    x.fork = f; x.join = j; x.s = st;      // published complete
    return &x;
}
// runs 0, 2, 4, ... of a split launch go to the side stream, the others stay on the caller's; join() orders the caller's stream behind the side stream
struct RunOverlap {
    SideStream* ss = nullptr; hipStream_t main; bool forked = false; unsigned idx = 0;
    RunOverlap(const troyn_plan* p, hipStream_t s, bool enable) : main(s) { if (enable && !p->opt.ntt_overlap_off) ss = side_stream(p->device); }
    hipStream_t next() {
        const bool side = ss && (idx++ & 1u) == 0u;
        if (!side) return main;
        if (!forked) {
            if (hipEventRecord(ss->fork, main) != hipSuccess || hipStreamWaitEvent(ss->s, ss->fork, 0) != hipSuccess) { (void)hipGetLastError(); ss = nullptr; return main; }
            forked = true;
        }
        return ss->s;
    }
    int join() {       // also on an error path: whatever was queued on the side stream keeps writing the caller's buffers
        if (!forked) return TROYN_OK;
        forked = false;
        if (hipEventRecord(ss->join, ss->s) == hipSuccess && hipStreamWaitEvent(main, ss->join, 0) == hipSuccess) return TROYN_OK;
        (void)hipGetLastError();
        const hipError_t e = hipStreamSynchronize(ss->s);      // fallback: the host waits for the side stream instead of the caller's stream
        if (e != hipSuccess) return fail((int)e, std::string("[RunOverlap::join] ") + hipGetErrorString(e));
        return TROYN_OK;
    }
    ~RunOverlap() { (void)join(); }
};
constexpr size_t OVERLAP_MIN_LIMB_POLYS = 512;      // per split launch (all runs together)
}  // namespace

static bool use_f64(const troyn_plan* p, unsigned table_start, unsigned table_count) {
    // FP64 butterflies when every modulus this launch can touch is below 2^50
    bool f64 = !force_integer_ntt(p) && p->log_n >= 10;
    for (unsigned i = 0; f64 && i < table_count; i++) f64 = p->small_modulus[table_start + i] != 0;
    return f64;
}

static inline const void* twiddles(const troyn_plan* p, bool f64, bool inverse) {
    if (f64) return inverse ? (const void*)p->d_inv_f64 : (const void*)p->d_fwd_f64;
    return inverse ? (const void*)p->d_inv : (const void*)p->d_fwd;
}
// what launch_ntt sets, for the launches of one arithmetic class that bypass it (inputs read once, no XCD grouping)
static inline void prep_direct(const troyn_plan* p, NttArgs& x, bool f64, bool inverse) {
    x.mods = p->d_mods; x.stream_loads = 1u; x.xcd_groups = 0u;
    x.tw = twiddles(p, f64, inverse);
}
// `next` reads what `prev` wrote (next may be prev itself: a second pass in place in its own output)
static inline void as_input_of(NttArgs& next, const NttArgs& prev) {
    next.in = prev.out; next.in_bstride = prev.out_bstride; next.in_pstride = prev.out_pstride; next.in_cstride = prev.out_cstride;
}

// The two notions of a limb's arithmetic class.  by_table: the modulus is below 2^50 (its FP64 twiddles exist); by_policy: it takes the FP64
// kernels now (also TROYN_NTT_ARITH=u64 and log_n >= 10).  They differ under TROYN_NTT_ARITH=u64: a by_table split of {60,40,40,60} still
// issues one launch per run, each on the integer kernels.
static inline bool class_by_table(const troyn_plan* p, unsigned mi) { return p->small_modulus[mi] != 0; }
static inline bool class_by_policy(const troyn_plan* p, unsigned mi) { return use_f64(p, mi, 1); }
template <typename Cls>
static inline bool one_class(const troyn_plan* p, unsigned table_start, unsigned count, Cls cls) {
    for (unsigned j = 1; j < count; j++) if (cls(p, table_start + j) != cls(p, table_start)) return false;
    return true;
}
// f(j0, j1, stream) once per run [j0, j1) of consecutive limbs of one class inside [table_start, table_start + count), j relative to table_start.
// overlap: runs of different classes in flight together (RunOverlap above; forked and joined here, also when f fails); a launch that is one
// run stays on the caller's stream.
template <typename Cls, typename F>
static int for_class_runs(const troyn_plan* p, unsigned table_start, unsigned count, Cls cls, bool overlap, hipStream_t s, F&& f) {
    RunOverlap ov(p, s, overlap);
    for (unsigned j0 = 0, j1; j0 < count; j0 = j1) {
        for (j1 = j0 + 1; j1 < count && cls(p, table_start + j1) == cls(p, table_start + j0); j1++) {}
        if (int rc = f(j0, j1, (j0 == 0 && j1 == count) ? s : ov.next())) return rc;
    }
    return ov.join();
}

static int launch_ntt(const troyn_plan* p, NttArgs a, size_t batch, bool inverse, hipStream_t s, u64* two_pass_scratch = nullptr) {
    a.mods = p->d_mods;
    // inputs shared by several limb-polynomials of the launch (stride 0) should stay cached
    a.stream_loads = ((a.pcount <= 1 || a.in_pstride != 0) && (a.ncomp <= 1 || a.in_cstride != 0)) ? 1u : 0u;
    const size_t lp = batch * a.pcount * a.ncomp;
    if (lp == 0) return TROYN_OK;
    // limbs that share one input row (component stride 0) are co-located on an XCD by the fused forward kernels
    a.xcd_groups = ((a.load_mode != NTT_LOAD_PLAIN || a.fused_mode == NTT_FUSED_TAIL_RESCALE || a.fused_mode == NTT_FUSED_TAIL_RESCALE_W) && a.in_cstride == 0 && a.ncomp > 1) ? (unsigned)(batch * a.pcount) : 0u;
    if (lp * ((size_t)1 << (p->log_n > 12 ? p->log_n - 12 : 0)) > 0x7fffffffull)
        return fail(TROYN_E_INVALID, "[troyn_ntt] batch too large for one launch");
    bool f64 = use_f64(p, a.table_start, a.table_count);
    if (!f64 && !force_integer_ntt(p) && p->log_n >= 10 && a.mode == TROYN_IDX_COMPONENTWISE && a.ncomp > 1 && a.ncomp <= a.table_count &&
        a.fused_mode == 0 && p->opt.ntt_split != 0 &&
        // (a launch that cannot fill the chip is latency-bound: one integer launch beats two half-empty ones -- one ciphertext at N = 16384
        // {60,50,50,50,50,60}: relinearize 102 -> 80 us, rescale 51 -> 40 us)
        (p->opt.ntt_split == 1 || !is_small_launch(lp)) &&
        ((a.load_mode == NTT_LOAD_PLAIN && a.store_mode == NTT_STORE_PLAIN && !two_pass_scratch) || p->log_n >= 14 || p->opt.ntt_split == 1 ||
         (!p->opt.ntt_overlap_off && lp >= OVERLAP_MIN_LIMB_POLYS))) {
        // A component-wise launch over limbs of both size classes ({60,40,40,60}: the reference's default chain): split it into
        // runs of one class, so that the limbs below 2^50 take the FP64 butterflies instead of following the 60-bit limbs into the
        // integer ones.  Limbs are independent; results are unchanged.  The launches with a fused prologue / epilogue (key-switch tail,
        // rescale) can split the same way (TROYN_NTT_SPLIT=1: their per-component operands move with the run, and the FP64 loader
        // reduces the word of a wide dropped prime with integer arithmetic first, ArithF64::load_io), but they run at the same ~3 TB/s
        // under either policy at N = 8192, so the extra launch only costs there: relinearize {60,40,40,60} 731 k split vs 749 k unsplit -- not the
        // default at N <= 8192.  N >= 16384 (round 5): the integer kernels are one 1024-thread workgroup per CU (whole-limb tiles) or two strided
        // passes, the FP64 ones run on half-word tiles: {60,50,50,50,50,60} key-switch tail 835 us unsplit for 512 items, i.e. 163 ns per row
        // against 83 ns -- split by default (TROYN_NTT_SPLIT=0: one integer launch).
        if (!one_class(p, a.table_start, a.ncomp, class_by_table))
            return for_class_runs(p, a.table_start, a.ncomp, class_by_table, lp >= OVERLAP_MIN_LIMB_POLYS, s, [&](unsigned j0, unsigned j1, hipStream_t rs) {
                NttArgs r = a;
                r.in = a.in + (long long)j0 * a.in_cstride; r.out = a.out + (long long)j0 * a.out_cstride;
                r.ncomp = j1 - j0; r.table_start = a.table_start + j0; r.table_count = j1 - j0;
                if (a.ext0) r.ext0 = a.ext0 + (long long)j0 * a.ext0_cstride;
                if (a.ext1) r.ext1 = a.ext1 + (long long)j0 * a.ext1_cstride;
                if (a.inv_table) r.inv_table = a.inv_table + j0;
                // (two-pass sizes: every run keeps its own part of the scratch -- the runs may be in flight together)
                u64* run_scratch = two_pass_scratch ? two_pass_scratch + batch * (size_t)a.pcount * j0 * p->n : nullptr;
                return launch_ntt(p, r, batch, inverse, rs, run_scratch);
            });
    }
    a.tw = twiddles(p, f64, inverse);
    if (!launch_transform(p->log_n, f64, a, lp, inverse, launch_ctx(p, s), two_pass_scratch)) {
        a.tw = twiddles(p, false, inverse);
        launch_ntt_generic(a, p->log_n, inverse, lp, launch_ctx(p, s));
    }
    LAUNCH_CHECK();
    return TROYN_OK;
}

// ---- tensor product of two 2-component ciphertexts fused with the transforms around it (tensor_core_kernel) ----
// two-pass sizes (N = 32768, 65536): stage 0 = first forward pass alone, stage 1 = last forward pass + tensor product + first inverse
// pass, stage 2 = last inverse pass.  Whole-limb sizes (N = 1024 .. 8192): stage 1 is everything.
// 0: limbs [0, ncomp) of plan p cannot take the fused tensor path; 1: whole-limb tiles; 2: two-pass transforms.  One arithmetic class.
static int tensor_path_kind(const troyn_plan* p, unsigned ncomp) {
    if (p->opt.tensor_split) return 0;   // TROYN_BFV_TENSOR=split: separate transform and dyadic launches (A/B runs, tests of that path)
    // whole-limb tiles; limbs of both classes: one launch per run of one class (tensor_stage).  N = 16384 holds three polynomials of
    // 16 coefficients per thread under the 128-register cap of a 1024-thread workgroup only with 78-93 spilled registers, and is
    // still 8 % faster than the separate launches (83.8 k vs 77.2 k products/s at 6 x 50-bit)
    if (p->log_n >= 10 && p->log_n <= 14) return 1;
    if (!one_class(p, 0, ncomp, class_by_table)) return 0;
    if (p->log_n == 15 || p->log_n == 16) return 2;
    return 0;
}
// one launch: limbs [j0, j1) of a, b, d, all of one class
static int tensor_stage_run(const troyn_plan* p, int stage, NttArgs a, NttArgs b, NttArgs d, unsigned j0, unsigned j1, size_t batch, hipStream_t s) {
    for (NttArgs* x : {&a, &b, &d}) {
        x->in += (long long)j0 * x->in_cstride; if (x->out) x->out += (long long)j0 * x->out_cstride;
        x->ncomp = j1 - j0; x->table_start += j0; x->table_count = j1 - j0;
    }
    const bool f64 = use_f64(p, a.table_start, a.ncomp);
    prep_direct(p, a, f64, stage == 2); prep_direct(p, b, f64, false); prep_direct(p, d, f64, true);
    if ((batch * a.pcount * a.ncomp) << (p->log_n > 12 ? p->log_n - 12 : 0) > 0x7fffffffull) return fail(TROYN_E_INVALID, "[troyn_ntt] batch too large for one launch");
    if (!launch_tensor(p->log_n, f64, stage, a, b, d, batch, launch_ctx(p, s)))
        return fail(TROYN_E_INVALID, "[troyn_bfv_multiply] no fused tensor kernel for this size");
    LAUNCH_CHECK();
    return TROYN_OK;
}
static int tensor_stage(const troyn_plan* p, int stage, const NttArgs& a, const NttArgs& b, const NttArgs& d, size_t batch, hipStream_t s) {
    // limbs of both arithmetic classes ({60,40,40,60}): one launch per run of limbs of one class (limbs are independent), one after the other
    return for_class_runs(p, a.table_start, a.ncomp, class_by_table, false, s,
                          [&](unsigned j0, unsigned j1, hipStream_t rs) { return tensor_stage_run(p, stage, a, b, d, j0, j1, batch, rs); });
}

static NttArgs contiguous_args(const troyn_plan* p, const u64* in, u64* out, size_t pcount, size_t ncomp,
                               unsigned table_start, unsigned table_count, int mode, unsigned decomp) {
    NttArgs a;
    std::memset(&a, 0, sizeof(a));
    a.in = in; a.out = out;
    a.in_cstride = a.out_cstride = p->n;
    a.in_pstride = a.out_pstride = (long long)ncomp * p->n;
    a.in_bstride = a.out_bstride = (long long)pcount * ncomp * p->n;
    a.pcount = (unsigned)pcount; a.ncomp = (unsigned)ncomp;
    a.table_start = table_start; a.table_count = table_count; a.mode = (unsigned)mode; a.decomp = decomp;
    return a;
}

extern "C" int troyn_ntt(const troyn_plan* plan, int inverse, const uint64_t* in, uint64_t* out,
                         size_t batch, size_t pcount, size_t ncomp,
                         uint32_t table_start, uint32_t table_count, int indexer_mode, uint32_t decomp_size,
                         troyn_stream_t stream) {
    select_device(plan);
    if (!plan || !in || !out) return fail(TROYN_E_INVALID, "[troyn_ntt] null argument");
    if (table_count == 0 || table_start + table_count > plan->K)
        return fail(TROYN_E_INVALID, "[troyn_ntt] table slice out of range");
    if (indexer_mode == TROYN_IDX_COMPONENTWISE && ncomp > table_count)
        return fail(TROYN_E_INVALID, "[troyn_ntt] more components than tables");
    if (indexer_mode == TROYN_IDX_KS_SET_PRODUCTS && (pcount > decomp_size + 1 || decomp_size >= table_count + 0u + 1u))
        return fail(TROYN_E_INVALID, "[troyn_ntt] bad KeySwitchingSetProducts shape");
    if (indexer_mode == TROYN_IDX_KS_SKIP_FINALS && (ncomp > decomp_size + 1 || decomp_size > table_count))
        return fail(TROYN_E_INVALID, "[troyn_ntt] bad KeySwitchingSkipFinals shape");
    NttArgs a = contiguous_args(plan, (const u64*)in, (u64*)out, pcount, ncomp, table_start, table_count, indexer_mode, decomp_size);
    return launch_ntt(plan, a, batch, inverse != 0, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------
// streaming ops
// ---------------------------------------------------------------------------------------
static inline unsigned chunks_pairs(unsigned n) { unsigned c = (n / 2 + POLY_BLOCK - 1) / POLY_BLOCK; return c ? c : 1; }
static inline unsigned chunks_single(unsigned n) { unsigned c = (n + 255) / 256; return c ? c : 1; }

static int check_rows(size_t rows, unsigned chunks) {
    if (rows * chunks > 0x7fffffffull) return fail(TROYN_E_INVALID, "[troyn] batch too large for one launch");
    return TROYN_OK;
}

template <int OP>
static int launch_elementwise(const troyn_plan* p, uint32_t mod_start, uint32_t nmod, const uint64_t* a, const uint64_t* b,
                              uint64_t scalar, uint64_t* out, size_t count, troyn_stream_t stream) {
    if (!p || !a || !out || (OP != EW_NEG && OP != EW_MULS && OP != EW_MOD && !b)) return fail(TROYN_E_INVALID, "[troyn elementwise] null argument");
    if (nmod == 0 || mod_start + nmod > p->K) return fail(TROYN_E_INVALID, "[troyn elementwise] modulus slice out of range");
    const size_t rows = count * nmod;
    if (rows == 0) return TROYN_OK;
    const unsigned ch = chunks_pairs(p->n);
    if (int rc = check_rows(rows, ch)) return rc;
    hipLaunchKernelGGL((elementwise_kernel<OP>), dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, (hipStream_t)stream,
                       ch, p->d_mods, mod_start, nmod, p->n, (const u64*)a, (const u64*)b, (u64)scalar, (u64*)out);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_add(const troyn_plan* p, uint32_t ms, uint32_t nm, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count, troyn_stream_t s) {
    select_device(p);
    return launch_elementwise<EW_ADD>(p, ms, nm, a, b, 0, out, count, s);
}
extern "C" int troyn_sub(const troyn_plan* p, uint32_t ms, uint32_t nm, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count, troyn_stream_t s) {
    select_device(p);
    return launch_elementwise<EW_SUB>(p, ms, nm, a, b, 0, out, count, s);
}
extern "C" int troyn_negate(const troyn_plan* p, uint32_t ms, uint32_t nm, const uint64_t* a, uint64_t* out, size_t count, troyn_stream_t s) {
    select_device(p);
    return launch_elementwise<EW_NEG>(p, ms, nm, a, nullptr, 0, out, count, s);
}
extern "C" int troyn_multiply_scalar(const troyn_plan* p, uint32_t ms, uint32_t nm, const uint64_t* a, uint64_t scalar, uint64_t* out, size_t count, troyn_stream_t s) {
    select_device(p);
    return launch_elementwise<EW_MULS>(p, ms, nm, a, nullptr, scalar, out, count, s);
}
extern "C" int troyn_dyadic_product(const troyn_plan* p, uint32_t ms, uint32_t nm, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count, troyn_stream_t s) {
    select_device(p);
    return launch_elementwise<EW_MUL>(p, ms, nm, a, b, 0, out, count, s);
}

extern "C" int troyn_modulo(const troyn_plan* p, uint32_t ms, uint32_t nm, const uint64_t* a, uint64_t* out, size_t count, troyn_stream_t s) {
    select_device(p);
    return launch_elementwise<EW_MOD>(p, ms, nm, a, nullptr, 0, out, count, s);
}
extern "C" int troyn_multiply_uint64operand(const troyn_plan* p, uint32_t ms, uint32_t nm, const uint64_t* a, const uint64_t* operands,
                                            uint64_t* out, size_t count, troyn_stream_t s) {
    select_device(p);
    return launch_elementwise<EW_MULOP>(p, ms, nm, a, operands, 0, out, count, s);
}

static int launch_convolute(const DevModulus* mods, unsigned n, uint32_t mod_start, uint32_t nmod,
                            const u64* a, size_t pa, const u64* b, size_t pb, u64* out, size_t batch, hipStream_t s) {
    const size_t rows = batch * nmod;
    if (rows == 0) return TROYN_OK;
    if (pa == 2 && pb == 2) {
        const unsigned ch = chunks_pairs(n);
        if (int rc = check_rows(rows, ch)) return rc;
        hipLaunchKernelGGL((dyadic_convolute_kernel<2, 2>), dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s, ch, mods, mod_start, nmod, n, a, b, out);
    } else if (pa == 3 && pb == 2) {
        const unsigned ch = chunks_pairs(n);
        if (int rc = check_rows(rows, ch)) return rc;
        hipLaunchKernelGGL((dyadic_convolute_kernel<3, 2>), dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s, ch, mods, mod_start, nmod, n, a, b, out);
    } else if (pa == 2 && pb == 3) {
        const unsigned ch = chunks_pairs(n);
        if (int rc = check_rows(rows, ch)) return rc;
        hipLaunchKernelGGL((dyadic_convolute_kernel<2, 3>), dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s, ch, mods, mod_start, nmod, n, a, b, out);
    } else {
        const unsigned ch = chunks_single(n);
        if (int rc = check_rows(rows, ch)) return rc;
        hipLaunchKernelGGL(dyadic_convolute_generic_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s, ch, mods, mod_start, nmod, n,
                           a, (unsigned)pa, b, (unsigned)pb, out);
    }
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_dyadic_convolute(const troyn_plan* p, uint32_t mod_start, uint32_t nmod,
                                      const uint64_t* a, size_t pa, const uint64_t* b, size_t pb, uint64_t* out,
                                      size_t batch, troyn_stream_t stream) {
    select_device(p);
    if (!p || !a || !b || !out) return fail(TROYN_E_INVALID, "[fgk::dyadic_convolute] null argument");
    if (nmod == 0 || mod_start + nmod > p->K) return fail(TROYN_E_INVALID, "[fgk::dyadic_convolute] modulus slice out of range");
    if (pa < 1 || pb < 1 || pa > 16 || pb > 16) return fail(TROYN_E_INVALID, "[fgk::dyadic_convolute] Result size mismatch");
    return launch_convolute(p->d_mods, p->n, mod_start, nmod, (const u64*)a, pa, (const u64*)b, pb, (u64*)out, batch, (hipStream_t)stream);
}

// SUM_t a[t] (x) b[t] into out (poly_kernels.hpp dyadic_convolute_accumulate_kernel): launches of at most CONV_ACC_MAX_TERMS terms, the tables
// by value in the kernel arguments (no upload, no host wait); every launch after the first carries `out`.  The caller has checked the tables.
static int launch_convolute_accumulate(const DevModulus* mods, unsigned n, uint32_t mod_start, uint32_t nmod, const uint64_t* const* a,
                                       const uint64_t* const* b, size_t terms, u64* out, int accumulate, size_t batch, hipStream_t s) {
    const size_t rows = batch * nmod;
    if (rows == 0) return TROYN_OK;
    const unsigned ch = chunks_pairs(n);
    if (int rc = check_rows(rows, ch)) return rc;
    for (size_t t0 = 0; t0 < terms; t0 += CONV_ACC_MAX_TERMS) {
        const unsigned cnt = (unsigned)std::min<size_t>(terms - t0, CONV_ACC_MAX_TERMS);
        ConvAccPtrs g;
        for (unsigned t = 0; t < CONV_ACC_MAX_TERMS; t++) {
            g.a[t] = reinterpret_cast<const u64*>(a[t0 + (t < cnt ? t : 0)]);
            g.b[t] = reinterpret_cast<const u64*>(b[t0 + (t < cnt ? t : 0)]);
        }
        const int carry = (accumulate || t0 > 0) ? 1 : 0;
        if (cnt >= 4)
            hipLaunchKernelGGL((dyadic_convolute_accumulate_kernel<4>), dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s, ch, mods, mod_start, nmod, n, g, cnt, out, carry);
        else
            hipLaunchKernelGGL((dyadic_convolute_accumulate_kernel<2>), dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s, ch, mods, mod_start, nmod, n, g, cnt, out, carry);
        LAUNCH_CHECK();
    }
    return TROYN_OK;
}

// argument checks shared by troyn_dyadic_convolute_accumulate and the chain entry built on it (P: the caller's name for the messages)
static int check_convolute_accumulate(const char* P, const troyn_plan* p, uint32_t mod_start, uint32_t nmod, const uint64_t* const* a,
                                      const uint64_t* const* b, size_t terms, const uint64_t* out, size_t out_words, size_t batch) {
    if (!p || !a || !b) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (terms == 0) return fail(TROYN_E_INVALID, std::string(P) + " no terms");
    if (nmod == 0 || (size_t)mod_start + nmod > p->K) return fail(TROYN_E_INVALID, std::string(P) + " modulus slice out of range");
    if (batch == 0) return TROYN_OK;
    if (!out) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if ((uintptr_t)out & 15) return fail(TROYN_E_INVALID, std::string(P) + " misaligned destination");
    const size_t in_bytes = batch * 2 * (size_t)nmod * p->n * sizeof(u64);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + out_words * sizeof(u64);
    for (size_t t = 0; t < terms; t++) {
        for (const uint64_t* q : {a[t], b[t]}) {
            if (!q || ((uintptr_t)q & 15)) return fail(TROYN_E_INVALID, std::string(P) + " null or misaligned pointer in the tables");
            if ((uintptr_t)q < o1 && o0 < (uintptr_t)q + in_bytes) return fail(TROYN_E_INVALID, std::string(P) + " out overlaps an input");
        }
    }
    return TROYN_OK;
}

extern "C" int troyn_dyadic_convolute_accumulate(const troyn_plan* p, uint32_t mod_start, uint32_t nmod,
                                                 const uint64_t* const* a, const uint64_t* const* b, size_t terms,
                                                 uint64_t* out, int accumulate, size_t batch, troyn_stream_t stream) {
    select_device(p);
    const char* P = "[troyn_dyadic_convolute_accumulate]";
    if (int rc = check_convolute_accumulate(P, p, mod_start, nmod, a, b, terms, out, batch * 3 * (size_t)nmod * (p ? p->n : 0), batch)) return rc;
    return launch_convolute_accumulate(p->d_mods, p->n, mod_start, nmod, a, b, terms, (u64*)out, accumulate, batch, (hipStream_t)stream);
}

// Scalar-weighted sums (poly_kernels.hpp scalar_weighted_sums_kernel).  The slot tile of a launch: the smallest instantiated tile that holds
// every slot, 8 beyond that.
static inline unsigned ssum_tile(size_t slots) { return slots > 4 ? 8u : slots > 2 ? 4u : slots > 1 ? 2u : 1u; }
// workspace: the scalars as [tile][limb][term][TS] (dead slots of the last tile zero), then the constants [slots][nmod]
static inline size_t ssum_scalar_words(size_t nmod, size_t terms, size_t slots) {
    const size_t ts = ssum_tile(slots);
    return (slots + ts - 1) / ts * ts * nmod * terms;
}

extern "C" size_t troyn_scalar_weighted_sums_workspace_bytes(const troyn_plan* p, uint32_t nmod, size_t terms, size_t slots) {
    (void)p;
    return (ssum_scalar_words(nmod, terms, slots) + slots * (size_t)nmod) * sizeof(u64);
}

template <int TS>
static void launch_scalar_sums_tile(unsigned blocks, hipStream_t s, unsigned ch, const DevModulus* mods, uint32_t mod_start, uint32_t nmod, unsigned n,
                                    const ScalarSumPtrs& g, unsigned cnt, const u64* scal, unsigned scal_terms, unsigned term0, const u64* consts,
                                    int at0, unsigned pcount, unsigned rows, unsigned slots, u64* out, int carry) {
    if (cnt >= 4)
        hipLaunchKernelGGL((scalar_weighted_sums_kernel<TS, 4>), dim3(blocks), dim3(POLY_BLOCK), 0, s, ch, mods, mod_start, nmod, n, g, cnt, scal, scal_terms,
                           term0, consts, at0, pcount, rows, slots, out, carry);
    else
        hipLaunchKernelGGL((scalar_weighted_sums_kernel<TS, 2>), dim3(blocks), dim3(POLY_BLOCK), 0, s, ch, mods, mod_start, nmod, n, g, cnt, scal, scal_terms,
                           term0, consts, at0, pcount, rows, slots, out, carry);
}

extern "C" int troyn_scalar_weighted_sums(const troyn_plan* p, uint32_t mod_start, uint32_t nmod, const uint64_t* const* in, const uint32_t* in_nmod,
                                          size_t terms, const uint64_t* scalars, const uint64_t* constants, int constant_at_index0, size_t pcount,
                                          uint64_t* out, size_t slots, size_t batch, void* workspace, size_t workspace_bytes, troyn_stream_t stream) {
    select_device(p);
    const std::string P = "[troyn_scalar_weighted_sums]";
    if (!p || !in || !in_nmod || !scalars) return fail(TROYN_E_INVALID, P + " null argument");
    if (terms == 0) return fail(TROYN_E_INVALID, P + " no terms");
    if (slots == 0) return fail(TROYN_E_INVALID, P + " no slots");
    if (pcount == 0) return fail(TROYN_E_INVALID, P + " no polynomials");
    if (nmod == 0 || (size_t)mod_start + nmod > p->K) return fail(TROYN_E_INVALID, P + " modulus slice out of range");
    if (terms > 0xffffffffull || slots > 0xffffffffull || pcount > 0xffffffffull) return fail(TROYN_E_INVALID, P + " table too large");
    for (size_t t = 0; t < terms; t++)
        if (in_nmod[t] < nmod) return fail(TROYN_E_INVALID, P + " an input has fewer limbs than nmod");
    for (size_t s = 0; s < slots; s++) {
        for (size_t l = 0; l < nmod; l++) {
            const u64 q = p->moduli[mod_start + l];
            for (size_t t = 0; t < terms; t++)
                if (scalars[(s * terms + t) * nmod + l] >= q) return fail(TROYN_E_INVALID, P + " a scalar is not a canonical residue");
            if (constants && constants[s * nmod + l] >= q) return fail(TROYN_E_INVALID, P + " a constant is not a canonical residue");
        }
    }
    if (batch == 0) return TROYN_OK;      // the host tables have been checked; nothing to launch, no device buffer or pointer entry is looked at
    if (!out || !workspace) return fail(TROYN_E_INVALID, P + " null argument");
    if (((uintptr_t)out & 15) || ((uintptr_t)workspace & 15)) return fail(TROYN_E_INVALID, P + " misaligned destination or workspace");
    const unsigned n = p->n;
    const size_t rows = batch * pcount * nmod;
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + slots * rows * n * sizeof(u64);
    for (size_t t = 0; t < terms; t++) {
        const uintptr_t q = (uintptr_t)in[t];
        if (!q || (q & 15)) return fail(TROYN_E_INVALID, P + " null or misaligned pointer in the table");
        if (q < o1 && o0 < q + batch * pcount * in_nmod[t] * (size_t)n * sizeof(u64)) return fail(TROYN_E_INVALID, P + " out overlaps an input");
    }
    if (workspace_bytes < troyn_scalar_weighted_sums_workspace_bytes(p, nmod, terms, slots)) return fail(TROYN_E_WORKSPACE, P + " workspace too small");
    const unsigned ts = ssum_tile(slots);
    const size_t tiles = (slots + ts - 1) / ts;
    const unsigned ch = chunks_pairs(n);
    if (rows > 0xffffffffull) return fail(TROYN_E_INVALID, "[troyn] batch too large for one launch");
    if (int rc = check_rows(tiles * rows, ch)) return rc;
    // the host tables are read here: one upload of the re-laid scalars and the constants into the workspace
    const size_t sw = ssum_scalar_words(nmod, terms, slots);
    std::vector<u64> tab(sw + (constants ? slots * (size_t)nmod : 0), 0);
    for (size_t s = 0; s < slots; s++)
        for (size_t t = 0; t < terms; t++)
            for (size_t l = 0; l < nmod; l++)
                tab[(((s / ts) * nmod + l) * terms + t) * ts + s % ts] = scalars[(s * terms + t) * nmod + l];
    if (constants) std::copy(constants, constants + slots * (size_t)nmod, tab.begin() + sw);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = upload_host_table(s, workspace, tab.data(), tab.size() * sizeof(u64))) return rc;
    const u64* d_scal = (const u64*)workspace;
    const u64* d_const = constants ? d_scal + sw : nullptr;
    const unsigned blocks = (unsigned)(tiles * rows * ch);
    for (size_t t0 = 0; t0 < terms; t0 += SSUM_MAX_TERMS) {
        const unsigned cnt = (unsigned)std::min<size_t>(terms - t0, SSUM_MAX_TERMS);
        ScalarSumPtrs g;
        for (unsigned t = 0; t < SSUM_MAX_TERMS; t++) {
            g.in[t] = reinterpret_cast<const u64*>(in[t0 + (t < cnt ? t : 0)]);
            g.in_nmod[t] = in_nmod[t0 + (t < cnt ? t : 0)];
        }
        const int carry = t0 > 0 ? 1 : 0;
        const u64* cst = t0 + cnt == terms ? d_const : nullptr;      // the constant goes in with the last launch, after its reduction
#define TROYN_SSUM_LAUNCH(TS) launch_scalar_sums_tile<TS>(blocks, s, ch, p->d_mods, mod_start, nmod, n, g, cnt, d_scal, (unsigned)terms, (unsigned)t0, cst, \
                                                          constant_at_index0 ? 1 : 0, (unsigned)pcount, (unsigned)rows, (unsigned)slots, (u64*)out, carry)
        if (ts == 8) TROYN_SSUM_LAUNCH(8);
        else if (ts == 4) TROYN_SSUM_LAUNCH(4);
        else if (ts == 2) TROYN_SSUM_LAUNCH(2);
        else TROYN_SSUM_LAUNCH(1);
#undef TROYN_SSUM_LAUNCH
        LAUNCH_CHECK();
    }
    return TROYN_OK;
}

extern "C" int troyn_dyadic_square(const troyn_plan* p, uint32_t mod_start, uint32_t nmod,
                                   const uint64_t* a, uint64_t* out, size_t batch, troyn_stream_t stream) {
    select_device(p);
    if (!p || !a || !out) return fail(TROYN_E_INVALID, "[fgk::dyadic_square] null argument");
    if (nmod == 0 || mod_start + nmod > p->K) return fail(TROYN_E_INVALID, "[fgk::dyadic_square] modulus slice out of range");
    const size_t rows = batch * nmod;
    if (rows == 0) return TROYN_OK;
    const unsigned ch = chunks_pairs(p->n);
    if (int rc = check_rows(rows, ch)) return rc;
    hipLaunchKernelGGL(dyadic_square_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, (hipStream_t)stream,
                       ch, p->d_mods, mod_start, nmod, p->n, (const u64*)a, (u64*)out);
    LAUNCH_CHECK();
    return TROYN_OK;
}

// ---------------------------------------------------------------------------------------
// key switching
// ---------------------------------------------------------------------------------------
// Shoup quotients of the evaluation keys for the integer inner product (ks_mac_kernel<ArithU64>, NttArgs::key_quo):
// out[j][row][i] = floor(keys[j][row][i] * 2^64 / q_row), EXACT (estimate from the Barrett ratio, corrected with the 128-bit remainder), so
// that a <digit, key> term is a lazy Shoup product in [0, 4q) instead of a 128-bit product and its Barrett reduction.  Once per call.
static __global__ __launch_bounds__(256) void ks_key_quotients_kernel(KeyPtrs keys, unsigned L, unsigned K, unsigned n, const DevModulus* mods, u64* out) {
    const size_t per_key = (size_t)2 * K * n, total = (size_t)L * per_key;
    for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const unsigned j = (unsigned)(p / per_key);
        const size_t w = p % per_key;
        const DevModulus md = mods[(w / n) % K];
        const u64 k = keys.p[j][w];
        u64 e = k * md.ratio_hi + mul_hi(k, md.ratio_lo);            // floor(k floor(2^128/q) / 2^64): the quotient or up to two below it (k < q)
        u128 rem = ((u128)k << 64) - (u128)e * md.q;
        while (rem >= md.q) { ++e; rem -= md.q; }
        out[p] = e;
    }
}

// workgroup order of ksmac2_kernel (TROYN_KS_ORDER=plain|item|row|band):
//   0 plain: workgroups of an item dealt round-robin to the XCDs
//   1 item:  all workgroups of an item on one XCD (digits L2-resident, keys from the Infinity Cache)
//   2 row:   one output row at a time on the whole chip (keys L2-resident, digits re-fetched per row)
//   3 band:  per XCD, two rows x as many items as fill its 64 workgroup slots (keys of the band L2-resident, digits fetched once per band);
//            needs the batch to be a multiple of 8 x 64 / (2 tiles per row) items.  Default for N >= 16384 where it applies.
static unsigned ksmac_order(const troyn_plan* p, size_t batch, unsigned log_n) {
    const int want = p->opt.ks_order;
    if (want == 0) return 0u;
    if (batch % 8 != 0) return 0u;
    if (want == 2) return 2u;
    if (want == 1) return 1u;
    const size_t tiles = log_n >= 13 ? (size_t)1 << (log_n - 13) : 1, band_items = 8 * (64 / (2 * tiles));
    if (batch % band_items != 0) return 1u;
    // measured (bench.py other_configs, band vs item): N = 32768 relinearize +8 %, N = 16384 +2 % (the launch itself -4 %), N = 8192 -2..-7 %
    // (a row's keys are 0.4 MB there: every row already fits in L2 under the item order)
    return (log_n >= 14 || want == 3) ? 3u : 1u;
}

// The digit-parallel form of the inner product (ksmac2 SPLITJ + ksmac_split_reduce_kernel) pays when the plain form would leave most of the
// chip idle: batch * rows * tiles workgroups walking L digits one after the other (a single N = 16384 ciphertext: 12 workgroups, 85 us).
// TROYN_KS_SPLIT=0 / 1 forces it off / on (A/B runs, tests); it needs L >= 2 and its slots in the workspace.
static bool ksmac_split_wanted(const troyn_plan* p, size_t batch, unsigned L, unsigned log_n) {
    const int e = p->opt.ks_split;
    // L <= 15: the reducer adds the L re-centred slots (|slot| <= p/2 + 1, p < 2^50) in plain doubles, exact below 2^53 (ksmac_split_reduce_kernel)
    if (e == 0 || L < 2 || L > 15 || log_n < 13 || log_n > 15) return false;
    const size_t wgs = batch * (L + 1) << (log_n - 13);
    if (batch > 64) return false;                      // small batches only (the slots cost L times the inner product's output)
    return e == 1 || wgs <= 128;
}
// slots of the digit-parallel form: provisioned exactly when a call of this shape would take it (both read the same switch)
static size_t ks_split_words(const troyn_plan* p, size_t batch, unsigned L, unsigned log_n) {
    return ksmac_split_wanted(p, batch, L, log_n) ? batch * L * 2 * (size_t)(L + 1) * ((size_t)1 << log_n) : 0;
}


// Single objects at N = 16384 under the FP64 policy: "INTT of one row, then a forward transform of `fw.ncomp` limbs whose loader reads that row"
// in three launches instead of four -- first inverse pass, mrr_quartet_load_kernel (last inverse layers + loader + first forward layers on the
// shared quartets, troyn_mrr_small.hip), last forward pass with the epilogue of `fw`.  pa: the first inverse pass (in -> out); iv.in = pa.out.
static bool small_tail_wanted(const troyn_plan* p, size_t limb_polys) {
    // (N = 32768 transforms are two-pass at every size; the merged form is taken for the same small launches)
    return p->log_n >= 13 && p->log_n <= 15 && !p->opt.mrr_small_off && (p->log_n == 15 || !p->opt.ntt_small_two_pass_off) && is_small_launch(limb_polys);
}
static int small_tail(const troyn_plan* p, bool f64, NttArgs pa, size_t pa_limb_polys, NttArgs fw, u64* between, size_t groups, hipStream_t s) {
    const LaunchCtx lc = launch_ctx(p, s);
    auto pass = [&](int which, const NttArgs& x, size_t lp) { launch_small_pass(p->log_n, f64, which, x, lp, lc); };
    prep_direct(p, pa, f64, true);
    pass(0, pa, pa_limb_polys);
    LAUNCH_CHECK();
    NttArgs iv = pa;
    as_input_of(iv, pa);
    prep_direct(p, fw, f64, false);
    NttArgs first = fw;                 // the pass in between: [group][limb][N], contiguous (the layout launch_two_pass gives a scratch buffer)
    const long long N = (long long)p->n;
    first.out = between; first.out_cstride = N; first.out_pstride = (long long)fw.ncomp * N; first.out_bstride = (long long)fw.pcount * fw.ncomp * N;
    launch_mrr_quartet_load(p->log_n, groups, iv, first, s, f64);
    LAUNCH_CHECK();
    NttArgs second = fw;
    as_input_of(second, first);
    second.reduce_input = 0;
    pass(1, second, groups * fw.ncomp);
    LAUNCH_CHECK();
    return TROYN_OK;
}

// A chain with moduli of 2^50 and more, a few ciphertexts: its one-launch inner products (ksmac2<WIDE> + ksmaci) loop over the L digits inside
// 2 .. 4 workgroups per item and have no digit-parallel form, so a launch that cannot fill the chip is one long chain (one ciphertext at
// N = 16384 {60,50,50,50,50,60}: 148 us of inner product).  The two-launch form -- (L + 1) L digit transforms, then the multiply-accumulate -- spreads
// the same work over L times the workgroups: relinearize of one ciphertext 214 -> 84 us (N = 16384), 140 -> 78 us (N = 8192 {60,40,40,60}); equal at
// 256 workgroups of the one-launch form (N = 16384: 32 items; N = 8192: ~100), which is where this rule hands over.  TROYN_KS_MAC=fused / split force either.
// The first-generation kernel of N = 1024 .. 4096 (one workgroup per output row looping over the L digits, no digit-parallel form either) hands over
// the same way below 128 workgroups: one ciphertext at N = 4096, relinearize 40 -> 31 us (4 x 36-bit), 59 -> 42 us ({50,55,50}).
static bool ks_small_mixed(const troyn_plan* p, unsigned L, size_t batch) {
    if (p->opt.ks_mac_fused) return false;
    if (p->log_n >= 10 && p->log_n <= 12) return batch * (size_t)(L + 1) <= 128;
    if (p->log_n < 13 || p->log_n > 15) return false;
    if (use_f64(p, 0, L) && use_f64(p, p->K - 1, 1)) return false;
    return (batch * (size_t)(L + 1) << (p->log_n - 13)) <= (p->log_n == 13 ? 384u : 256u);      // (N = 8192: equal at ~400, 96 items of {60,40,40,60})
}

// Output rows k = 0 .. L of the inner product (row L: the special prime) by arithmetic class, as bit masks; wide_digits: some digit limb is 2^50
// or wider.  Computed ONCE per call and passed down: key preparation and launch must agree on the rows.
struct KsRows { unsigned long long small, wide; bool wide_digits; };
static KsRows ks_rows(const troyn_plan* p, unsigned L) {
    KsRows r{0, 0, false};
    for (unsigned k = 0; k <= L; k++) {
        const bool f64 = class_by_policy(p, k == L ? p->K - 1 : k);
        (f64 ? r.small : r.wide) |= 1ull << k;
        if (k < L && !f64) r.wide_digits = true;
    }
    return r;
}

// Argument blocks of the second-generation inner products, what every caller shares; call sites add diag*, ten_*, row_mask / no_load_corr and the
// digit-parallel part / raw fields.
static KsMacArgs ksmac2_args(const troyn_plan* p, unsigned L, size_t batch, const u64* digits, long long dig_bstride, u64* poly_prod, const double* keys) {
    const unsigned K = p->K, n = p->n;
    KsMacArgs a;
    std::memset(&a, 0, sizeof(a));
    a.digits = digits; a.dig_bstride = dig_bstride; a.dig_cstride = n;
    a.out = poly_prod; a.out_bstride = 2ll * (L + 1) * n; a.out_pstride = (long long)(L + 1) * n; a.out_cstride = n;
    a.mods = p->d_mods; a.tw = p->d_fwd_f64; a.tw_r1 = p->d_fwd_r1; a.tw_r2 = p->d_fwd_r2;
    a.keys = keys; a.key_jstride = 2ll * K * n; a.key_pstride = (long long)K * n;
    a.L = L; a.table_start = 0; a.table_count = K; a.batch = (unsigned)batch;
    a.grouped = ksmac_order(p, batch, p->log_n);
    return a;
}
// rows: the rows of moduli >= 2^50 (KsRows::wide, never 0); keys: their (key, quotient) pairs [L][2][slots][N], then the diagonal blocks [slots][2][N]
static KsMacIArgs ksmaci_args(const troyn_plan* p, unsigned L, size_t batch, const u64* digits, long long dig_bstride, u64* poly_prod, const ulonglong2* keys,
                              unsigned long long rows) {
    const unsigned K = p->K, n = p->n, slots = (unsigned)__builtin_popcountll(rows);
    KsMacIArgs m;
    std::memset(&m, 0, sizeof(m));
    m.digits = digits; m.dig_bstride = dig_bstride; m.dig_cstride = n;
    m.out = poly_prod; m.out_bstride = 2ll * (L + 1) * n; m.out_pstride = (long long)(L + 1) * n; m.out_cstride = n;
    m.mods = p->d_mods; m.tw = p->d_fwd; m.tw_r1 = p->d_fwd_r1i; m.tw_r2 = p->d_fwd_r2i;
    m.keys = keys; m.key_jstride = 2ll * slots * n; m.key_pstride = (long long)slots * n;
    m.diag_keys = keys + (size_t)L * 2 * slots * n;
    m.L = L; m.table_start = 0; m.table_count = K; m.batch = (unsigned)batch;
    m.grouped = (batch % 8 == 0 && p->opt.ks_order != 0) ? 1u : 0u;
    m.row_mask = rows;
    return m;
}
// Keys of ksmac2_kernel, once per call: exact doubles in the accumulators' layout [L][2][K][N]; want_diag: the block (key j, modulus j) a second
// time in natural order behind them (DG / TEN epilogues).  scale_rows != 0 (fused chain): the rows r < scale_rows carry the factor qk^-1 mod q_r.
static int prepare_keys_f64(const troyn_plan* p, const KeyPtrs& kp, unsigned L, double* kf, unsigned scale_rows, bool want_diag, hipStream_t s) {
    const unsigned K = p->K, n = p->n;
    const size_t pairs = (size_t)L * 2 * K * (n / 2);
    launch_ksmac_prepare_keys(kp, L, 2 * K, n, kf, (unsigned)std::min<size_t>((pairs + 255) / 256, 4096), s,
                              scale_rows ? p->d_inv_last + (size_t)K * K : nullptr, scale_rows ? p->d_mods : nullptr, scale_rows,
                              want_diag ? kf + (size_t)L * 2 * K * n : nullptr);
    LAUNCH_CHECK();
    return TROYN_OK;
}
// Keys of ksmaci_kernel, once per call: (key, Shoup quotient) pairs of exactly the rows in `rows`, in the accumulators' layout; want_diag: their
// diagonal blocks in natural order behind them.  scale_rows as above.
static int prepare_keys_int(const troyn_plan* p, const KeyPtrs& kp, unsigned L, unsigned long long rows, ulonglong2* ki, unsigned scale_rows, bool want_diag,
                            hipStream_t s) {
    const unsigned K = p->K, n = p->n;
    const size_t words = (size_t)L * 2 * (unsigned)__builtin_popcountll(rows) * n;
    launch_ksmaci_prepare_keys(kp, L, K, n, rows, ki, (unsigned)std::min<size_t>((words + 255) / 256, 4096), s,
                               scale_rows ? p->d_inv_last + (size_t)K * K : nullptr, p->d_mods, scale_rows, want_diag ? ki + words : nullptr);
    LAUNCH_CHECK();
    return TROYN_OK;
}
// INTT of the two special-prime rows of poly_prod [item][2][L+1][N] into dst [item][2][N]
static NttArgs special_rows_args(const troyn_plan* p, const u64* poly_prod, u64* dst, unsigned L, unsigned comps = 2) {
    const unsigned n = p->n;
    NttArgs a = contiguous_args(p, poly_prod + (size_t)L * n, dst, comps, 1, p->K - 1, 1, TROYN_IDX_COMPONENTWISE, 0);
    a.in_pstride = (long long)(L + 1) * n; a.in_bstride = 2ll * (L + 1) * n;
    return a;
}

// (N >= 8192: the half-tile kernels, whose grid is up to 4 (L + 2) workgroups per item; the first-generation whole-limb kernel stays the path
// of N = 1024 .. 4096 -- its N = 8192 / 16384 instantiations left the library in round 5)
static int ks_mac_generation(const troyn_plan* p) { return p->log_n >= 13 ? 2 : 1; }

struct KsLayout {
    size_t target_intt, temp_ntt, poly_prod, prod_intt, temp_last, keys_f64, split, keys_quo, total;  // element offsets
};

static KsLayout ks_layout(const troyn_plan* p, unsigned L, size_t batch) {
    const size_t n = p->n;
    const bool gen2 = ks_mac_generation(p) == 2;
    KsLayout w;
    size_t off = 0;
    w.target_intt = off; off += batch * L * n;
    w.temp_ntt = off;    off += batch * (size_t)(L + 1) * L * n;
    w.poly_prod = off;   off += batch * 2 * (size_t)(L + 1) * n;
    w.prod_intt = off;   off += batch * 2 * (size_t)(L + 1) * n;
    w.temp_last = off;   off += batch * 2 * (size_t)L * n;
    w.keys_f64 = off;    off += (size_t)L * 2 * p->K * n + (size_t)L * 2 * n;     // prepared keys of ksmac2_kernel + the diagonal blocks in natural order
    w.split = off;       off += ks_split_words(p, batch, L, p->log_n);                        // slots of the digit-parallel inner product (small batches)
    // Shoup quotients of the keys for the integer inner product: chains with a modulus of 2^50 or more on the whole-limb sizes
    // (N >= 8192: (key, quotient) pairs of the wide rows in the accumulators' layout + the diagonal blocks in natural order, ksmaci_kernel)
    w.keys_quo = off;    off += (p->log_n >= 10 && p->log_n <= 15 && !use_f64(p, 0, p->K)) ? (size_t)L * 2 * p->K * n * (gen2 ? 2 : 1) + (gen2 ? (size_t)p->K * 2 * n * 2 : 0) : 0;
    w.total = off;
    return w;
}

extern "C" size_t troyn_switch_key_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t batch) {
    if (!plan) return 0;
    return ks_layout(plan, L, batch).total * sizeof(u64);
}
extern "C" size_t troyn_relinearize_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t batch) {
    return troyn_switch_key_workspace_bytes(plan, L, batch);
}

// BGV divides by the special prime with a correction computed mod t (ski_util5); everything before the tail is shared.
struct BgvTail { DevModulus t; u64 inv_special_mod_t; };

static bool coeff_tail_fused(const troyn_plan* p) { return !p->opt.ks_tail_split; }   // TROYN_KS_TAIL=split: inverse transforms and ski_util7 in separate launches

// The launches a key switch of one shape takes, decided ONCE per call; the steps below only read it, and ks_layout provisions from the same
// predicates (ks_split_words, ks_mac_generation).  Inner product: ksmac2 for every row | ksmac2<WIDE> + ksmaci | ks_mac_kernel | two launches.
enum KsMacForm { KS_MAC_F64, KS_MAC_MIXED, KS_MAC_GEN1, KS_MAC_TWO_LAUNCH };
enum KsTailForm { KS_TAIL_SMALL, KS_TAIL_NTT_FUSED, KS_TAIL_COEFF_FUSED, KS_TAIL_UNFUSED };
struct KsPath {
    bool fused;         // the optimised NTT kernels carry fused prologues / epilogues; tiny rings (generic kernel) and BGV use the unfused chain
    KsMacForm mac;
    bool dg;            // NTT-form target: the diagonal digit is applied in ksmac2's epilogue (DG), from the block (key j, modulus j) in natural order
    bool split;         // the digit-parallel form of ksmac2 (small launches)
    KsTailForm tail;
};
static KsPath ks_path(const troyn_plan* p, unsigned L, size_t batch, bool is_ntt_form, bool bgv) {
    KsPath k;
    k.fused = is_ntt_form && p->log_n >= 10 && !bgv;
    const bool two_launch = p->opt.ks_mac_split || ks_small_mixed(p, L, batch);
    // (2)+(3) in ONE launch for whole-limb rings (N <= 16384): every workgroup owns one output row of one item,
    //     transforms that row's L digits one after the other and multiplies them into register accumulators with
    //     the key (kernel_set_accumulate + ntt + kernel_accumulate_products, fgk/switch_key.cu:6-154); the
    //     (L+1)*L transformed digits never reach HBM.
    // (the band order pads an odd row count with one row of workgroups that exit: the grid guard counts L + 2 rows)
    const bool one_launch = !two_launch && p->log_n >= 10 && p->log_n <= 15 && batch * (size_t)(L + 1) <= 0x7fffffffull &&
                            (p->log_n <= 12 || (p->d_fwd_r2 && p->d_fwd_r2i && L + 1 <= 64 && batch * (size_t)(L + 2) * 4 <= 0x7fffffffull));
    k.mac = !one_launch ? KS_MAC_TWO_LAUNCH : ks_mac_generation(p) == 1 ? KS_MAC_GEN1 : use_f64(p, 0, p->K) ? KS_MAC_F64 : KS_MAC_MIXED;
    // The switch is read ONCE per call: the preparation and the instantiation choice must agree.
    k.dg = is_ntt_form && !p->opt.ks_diag_loop;
    // the digit-parallel form reads the caller's keys as they are, so its diagonal digit can only live in the epilogue
    k.split = k.mac == KS_MAC_F64 && ksmac_split_wanted(p, batch, L, p->log_n) && (k.dg || !is_ntt_form);
    if (k.fused) k.tail = small_tail_wanted(p, batch * 2 * L) ? KS_TAIL_SMALL : KS_TAIL_NTT_FUSED;
    else k.tail = (!is_ntt_form && !bgv && p->log_n >= 10 && p->log_n <= 17 && coeff_tail_fused(p)) ? KS_TAIL_COEFF_FUSED : KS_TAIL_UNFUSED;
    return k;
}

// one validated call; target: [batch] items of L limbs, `target_bstride` elements apart
struct KsCall {
    const troyn_plan* p; unsigned L; int is_ckks; bool is_ntt_form;
    const u64* target; size_t target_bstride; int assign_method;
    u64* dest; const u64* addend; size_t addend_bstride;
    u64* ws; KsLayout w; size_t batch; hipStream_t s; const BgvTail* bgv;
    const u64* digits; size_t digits_bstride;      // the target in coefficient form: the caller's rows, or target_intt after ks_digits
    // the tail's polynomials per item: 2 = both components of poly_prod [item][2][L+1][N] into dest [item][2][L][N]; 1 = component 1 alone into
    // dest [item][L][N] (the inner division of the double-hoisted BSGS transform; the items of poly_prod stay 2 (L+1) N apart)
    unsigned comps = 2;
};
// the first polynomial of poly_prod the tail divides
static u64* ks_tail_prod(const KsCall& c) { return c.ws + c.w.poly_prod + (c.comps == 1 ? (size_t)(c.L + 1) * c.p->n : 0); }

// (1) NTT form: bring the target back to coefficient form (evaluator_keyswitching_core.cu:817-821)
static int ks_digits(KsCall& c) {
    if (!c.is_ntt_form) return TROYN_OK;
    NttArgs a = contiguous_args(c.p, c.target, c.ws + c.w.target_intt, 1, c.L, 0, c.L, TROYN_IDX_COMPONENTWISE, 0);
    a.in_bstride = (long long)c.target_bstride;
    c.digits = c.ws + c.w.target_intt; c.digits_bstride = (size_t)c.L * c.p->n;
    return launch_ntt(c.p, a, c.batch, true, c.s);
}

// ksmac2_kernel: tiles of 2^13 outputs, two workgroups per CU, keys prepared once per call (ksmac_kernels.hpp)
static int ks_mac_f64(const KsCall& c, const KeyPtrs& kp, const KsPath& path) {
    const troyn_plan* p = c.p; const unsigned L = c.L, K = p->K, n = p->n;
    double* kf = reinterpret_cast<double*>(c.ws + c.w.keys_f64);
    // the digit-parallel form (small launches) reads the caller's keys as they are: no preparation pass
    if (!path.split) if (int rc = prepare_keys_f64(p, kp, L, kf, 0, path.dg, c.s)) return rc;
    KsMacArgs a = ksmac2_args(p, L, c.batch, c.digits, (long long)c.digits_bstride, c.ws + c.w.poly_prod, kf);
    a.diag = c.is_ntt_form ? c.target : nullptr; a.diag_bstride = (long long)c.target_bstride; a.diag_cstride = n;
    if (path.dg) a.diag_keys = kf + (size_t)L * 2 * K * n;
    {
        TimerScope ts(TROYN_TIMER_KS_INNER_PRODUCT, c.s);
        if (path.split) {
            a.grouped = 0;
            a.part = reinterpret_cast<double*>(c.ws + c.w.split); a.part_jstride = (long long)c.batch * a.out_bstride;
            a.split_skip_diag = path.dg ? 1u : 0u;
            a.raw = kp; a.raw_pstride = (long long)K * n;
            launch_ksmac2_split(p->log_n, c.batch, a, c.s, false, path.dg ? 2 : 0);
        } else launch_ksmac2(p->log_n, c.batch, L + 1, a, c.s);
    }
    LAUNCH_CHECK();
    return TROYN_OK;
}
// A chain with moduli of 2^50 and more (the reference's default {60,40,40,60}; {60,50,...,60} CKKS chains): the output rows of the
// moduli below 2^50 take ksmac2_kernel (exact FP64 butterflies; digits of wider limbs are reduced while loading), the rows of the wide
// moduli the integer kernel of the same shape (ksmaci_kernel, N = 8192 / 16384 / 32768; round 5).  Rows are independent; results are
// unchanged.  TROYN_NTT_ARITH=u64 sends every row to the integer kernel; N < 8192 keeps the first-generation kernel.
static int ks_mac_mixed(const KsCall& c, const KeyPtrs& kp, const KsPath& path) {
    const troyn_plan* p = c.p; const unsigned L = c.L, K = p->K, n = p->n;
    const KsRows rows = ks_rows(p, L);
    TimerScope ts(TROYN_TIMER_KS_INNER_PRODUCT, c.s);
    if (rows.small) {
        double* kf = reinterpret_cast<double*>(c.ws + c.w.keys_f64);
        // NTT-form target: the diagonal digit in the epilogue (DG) as in the all-FP64 path -- needs the diagonal key blocks in natural order
        if (int rc = prepare_keys_f64(p, kp, L, kf, 0, path.dg, c.s)) return rc;
        KsMacArgs m = ksmac2_args(p, L, c.batch, c.digits, (long long)c.digits_bstride, c.ws + c.w.poly_prod, kf);
        m.diag = c.is_ntt_form ? c.target : nullptr; m.diag_bstride = (long long)c.target_bstride; m.diag_cstride = n;
        if (path.dg) m.diag_keys = kf + (size_t)L * 2 * K * n;
        m.row_mask = rows.small;
        launch_ksmac2(p->log_n, c.batch, (unsigned)__builtin_popcountll(rows.small), m, c.s, false, rows.wide_digits);
        LAUNCH_CHECK();
    }
    // (no wide row: every row this level touches is narrow although the chain holds a wide modulus elsewhere -- ksmac2 above took all of them)
    if (rows.wide) {
        // integer rows: (key, Shoup quotient) pairs of exactly these rows, in the accumulators' layout, once per call
        ulonglong2* ki = reinterpret_cast<ulonglong2*>(c.ws + c.w.keys_quo);
        if (int rc = prepare_keys_int(p, kp, L, rows.wide, ki, 0, c.is_ntt_form, c.s)) return rc;
        KsMacIArgs m = ksmaci_args(p, L, c.batch, c.digits, (long long)c.digits_bstride, c.ws + c.w.poly_prod, ki, rows.wide);
        m.diag = c.is_ntt_form ? c.target : nullptr; m.diag_bstride = (long long)c.target_bstride; m.diag_cstride = n;
        launch_ksmaci(p->log_n, c.batch, m, c.s, c.is_ntt_form ? 1 : 0);
        LAUNCH_CHECK();
    }
    return TROYN_OK;
}
// the first-generation kernel: one workgroup per output row of an item, either arithmetic class
static int ks_mac_gen1(const KsCall& c, const KeyPtrs& kp) {
    const troyn_plan* p = c.p; const unsigned L = c.L, K = p->K, n = p->n;
    TimerScope ts(TROYN_TIMER_KS_INNER_PRODUCT, c.s);
    NttArgs a = contiguous_args(p, c.digits, c.ws + c.w.poly_prod, 1, L + 1, 0, K, TROYN_IDX_KS_SET_PRODUCTS, L);
    a.in_bstride = (long long)c.digits_bstride; a.in_pstride = 0; a.in_cstride = n;
    a.out_bstride = 2ll * (L + 1) * n; a.out_pstride = (long long)(L + 1) * n; a.out_cstride = n;
    a.reduce_input = 1;
    a.stream_loads = 0;                      // the L+1 rows of an item re-read the same digits
    a.skip_diag = c.is_ntt_form ? 1 : 0;     // digit k of row k is the NTT-form input limb itself
    a.ext0 = c.target; a.ext0_bstride = (long long)c.target_bstride; a.ext0_cstride = n;
    a.batch = (unsigned)c.batch; a.key_pstride = (long long)K * n;
    // rows of an item co-scheduled per XCD: all L+1 by default (the item's digits are then fetched once per XCD instead of
    // once per row; measured 1265 vs 1310 us per 512-item launch at cfg3), TROYN_KS_ROWS=1 restores plain row-major order
    const unsigned R = p->opt.ks_rows > 0 ? (unsigned)p->opt.ks_rows : L + 1;
    a.xcd_groups = (R > 1 && c.batch % 8 == 0 && (L + 1) % R == 0) ? R : 0u;
    a.mods = p->d_mods;
    const bool f64 = use_f64(p, 0, K);
    a.tw = twiddles(p, f64, false);
    if (!f64 && !p->opt.ks_mac_shoup_off) {
        // integer policy: the keys' Shoup quotients, once per call (TROYN_KS_MAC_SHOUP=0: Barrett-128 terms as in rounds 1-3; A/B, tests)
        u64* kq = c.ws + c.w.keys_quo;
        const size_t words = (size_t)L * 2 * K * n;
        hipLaunchKernelGGL(ks_key_quotients_kernel, dim3((unsigned)std::min<size_t>((words + 255) / 256, 4096)), dim3(256), 0, c.s, kp, L, K, n, p->d_mods, kq);
        LAUNCH_CHECK();
        a.key_quo = kq; a.key_quo_jstride = 2ll * K * n;
    }
    launch_ks_mac(p->log_n, f64, a, kp, c.batch * (size_t)(L + 1), launch_ctx(p, c.s));
    LAUNCH_CHECK();
    return TROYN_OK;
}
// (2) digit decomposition fused into the forward NTT (replaces kernel_set_accumulate, fgk/switch_key.cu:6-54,
//     + ntt_inplace_ps with key_switching_set_products, :907-908): temp_ntt [item][L+1][L][N], row i = digits reduced mod q_key(i)
static int ks_transform_digits(const KsCall& c, bool skip_diag) {
    const troyn_plan* p = c.p; const unsigned L = c.L;
    NttArgs a = contiguous_args(p, c.digits, c.ws + c.w.temp_ntt, L + 1, L, 0, p->K, TROYN_IDX_KS_SET_PRODUCTS, L);
    a.in_bstride = (long long)c.digits_bstride;
    a.in_pstride = 0;                 // every row re-reads the same L digits
    a.reduce_input = 1;
    a.skip_diag = skip_diag ? 1 : 0;  // row i, digit i is the NTT-form input itself: not recomputed
    return launch_ntt(p, a, c.batch, false, c.s);
}
static int ks_mac_two_launch(const KsCall& c, const KeyPtrs& kp, const KsPath& path) {
    const troyn_plan* p = c.p; const unsigned L = c.L, K = p->K, n = p->n;
    if (int rc = ks_transform_digits(c, path.fused)) return rc;
    // (3) <digits, key> inner product (fgk/switch_key.cu:83-154)
    const unsigned ch = chunks_pairs(n);
    const size_t rows = c.batch * (L + 1);
    if (int rc = check_rows(rows, ch)) return rc;
    hipLaunchKernelGGL(ks_accumulate_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, c.s,
                       ch, p->d_mods, K, L, n, c.ws + c.w.temp_ntt, kp, c.ws + c.w.poly_prod,
                       path.fused ? c.target : (const u64*)nullptr, c.target_bstride);
    LAUNCH_CHECK();
    return TROYN_OK;
}
// (2)+(3): poly_prod [item][2][L+1][N] = <digits, keys> in NTT form
static int ks_inner_product(const KsCall& c, const KeyPtrs& kp, const KsPath& path) {
    if (path.mac == KS_MAC_F64) return ks_mac_f64(c, kp, path);
    if (path.mac == KS_MAC_MIXED) return ks_mac_mixed(c, kp, path);
    return path.mac == KS_MAC_GEN1 ? ks_mac_gen1(c, kp) : ks_mac_two_launch(c, kp, path);
}
// (5)-(7) in ONE launch: the forward NTT reads the INTT'd special rows `src` [item][2][N] through the rounding-fix prologue (ski_util6_merged) and
// finishes with the divide-by-special-prime / assign epilogue (ski_util7_merged)
static NttArgs ks_ntt_tail_args(const KsCall& c, const u64* src) {
    const troyn_plan* p = c.p; const unsigned L = c.L, K = p->K, n = p->n;
    NttArgs a = contiguous_args(p, src, c.dest, c.comps, L, 0, L, TROYN_IDX_COMPONENTWISE, 0);
    a.in_bstride = (long long)c.comps * n; a.in_pstride = n; a.in_cstride = 0;
    a.load_mode = NTT_LOAD_KS_ROUND; a.aux_mod = K - 1;
    a.store_mode = NTT_STORE_KS_FINISH;
    a.flags = (c.is_ckks ? 1u : 0u) | ((unsigned)c.assign_method << 1);
    a.ext0 = ks_tail_prod(c); a.ext0_bstride = 2ll * (L + 1) * n; a.ext0_pstride = (long long)(L + 1) * n; a.ext0_cstride = n;
    a.ext1 = c.addend; a.ext1_bstride = (long long)c.addend_bstride; a.ext1_pstride = (long long)L * n; a.ext1_cstride = n;
    a.inv_table = p->d_inv_last + (size_t)K * K;
    return a;
}
// a few ciphertexts at N = 16384: first inverse pass of the special rows in place (nothing else reads them), then the strided passes of both
// transforms as one launch (small_tail)
static int ks_tail_small(const KsCall& c) {
    const troyn_plan* p = c.p;
    const bool tail_f64 = use_f64(p, 0, c.L) && use_f64(p, p->K - 1, 1);      // else both transforms on the integer kernels (small launches are not split by class)
    u64* special = ks_tail_prod(c) + (size_t)c.L * p->n;
    NttArgs pa = special_rows_args(p, ks_tail_prod(c), special, c.L, c.comps);
    pa.out_pstride = pa.in_pstride; pa.out_bstride = pa.in_bstride;
    return small_tail(p, tail_f64, pa, c.batch * c.comps, ks_ntt_tail_args(c, c.ws + c.w.prod_intt), c.ws + c.w.temp_last, c.batch * c.comps, c.s);
}
// (4) INTT of only the special-prime rows, the result stays in NTT form (:991-996); then (5)-(7) as one launch
static int ks_tail_ntt_fused(const KsCall& c) {
    u64* spec = c.ws + c.w.prod_intt;
    if (int rc = launch_ntt(c.p, special_rows_args(c.p, ks_tail_prod(c), spec, c.L, c.comps), c.batch, true, c.s)) return rc;
    // N >= 32768 transforms in two passes: the pass in between goes to temp_last (unused on this path), never to dest
    return launch_ntt(c.p, ks_ntt_tail_args(c, spec), c.batch, false, c.s, c.ws + c.w.temp_last);
}
// coefficient form: INTT of the two special-prime rows, then the INTT of the 2L data rows finishes the key switch in its epilogue
// ((5) + (7), ski_util6_merged / ski_util7_merged) and writes the destination -- the INTT'd rows never reach HBM
static int ks_tail_coeff_fused(const KsCall& c) {
    const troyn_plan* p = c.p; const unsigned L = c.L, K = p->K, n = p->n;
    u64* spec = c.ws + c.w.prod_intt;
    if (int rc = launch_ntt(p, special_rows_args(p, ks_tail_prod(c), spec, L, c.comps), c.batch, true, c.s)) return rc;
    NttArgs f = contiguous_args(p, ks_tail_prod(c), c.dest, c.comps, L, 0, K, TROYN_IDX_COMPONENTWISE, 0);
    f.in_pstride = (long long)(L + 1) * n; f.in_bstride = 2ll * (L + 1) * n;
    f.load_mode = NTT_LOAD_KS_ROUND; f.aux_mod = K - 1;      // constants of the rounding fix (no forward prologue runs)
    f.store_mode = NTT_STORE_KS_FINISH;
    f.flags = (c.is_ckks ? 1u : 0u) | ((unsigned)c.assign_method << 1);
    f.in2 = spec; f.in2_bstride = (long long)c.comps * n; f.in2_pstride = n;
    f.ext0 = c.dest; f.ext0_bstride = (long long)c.comps * L * n; f.ext0_pstride = (long long)L * n; f.ext0_cstride = n;   // unused by this epilogue
    f.ext1 = c.addend; f.ext1_bstride = (long long)c.addend_bstride; f.ext1_pstride = (long long)L * n; f.ext1_cstride = n;
    f.inv_table = p->d_inv_last + (size_t)K * K;
    // two-pass sizes: the pass in between goes to the free part of prod_intt, never to dest (AddInplace reads the old destination)
    return launch_ntt(p, f, c.batch, true, c.s, spec + c.batch * 2 * (size_t)n);
}
// The NTT-form tails that correct before they divide (ks_tail_unfused, bgv_hoist_tail) make ONE use of the key-switch regions, comps <= 2: the special
// rows in coefficient form lead prod_intt ([batch][2][N]), the per-limb corrections follow them ([batch][2][L][N]: the region holds 2 (L + 1) rows per
// item), and temp_last ([batch][2][L][N]) takes their forward transform.  Every layout that feeds a tail (ks_workspace, hoist_layout, the sum_each and
// BSGS layouts) sizes the two regions as batch * 2 * (L + 1) * n and batch * 2 * L * n words; both tails take the corrections' place from here.
static inline u64* ks_ntt_correction_rows(const KsCall& c) { return c.ws + c.w.prod_intt + c.batch * 2 * (size_t)c.p->n; }
// steps (4)-(7) as separate launches: tiny rings, BGV, TROYN_KS_TAIL=split
static int ks_tail_unfused(const KsCall& c) {
    const troyn_plan* p = c.p; const unsigned L = c.L, K = p->K, n = p->n;
    const bool ntt = c.is_ntt_form;
    const size_t batch = c.batch, rows = batch * c.comps * L;
    const unsigned ch = c.bgv ? chunks_single(n) : chunks_pairs(n);
    hipStream_t s = c.s;
    u64* prod_intt = c.ws + c.w.prod_intt;
    u64* temp_last = c.ws + c.w.temp_last;
    int rc;
    // (4) INTT: only the special-prime rows when the result stays in NTT form; all rows otherwise (:991-996)
    if (ntt) rc = launch_ntt(p, special_rows_args(p, ks_tail_prod(c), prod_intt, L, c.comps), batch, true, s);
    else {
        NttArgs iv = contiguous_args(p, ks_tail_prod(c), prod_intt, c.comps, L + 1, 0, K, TROYN_IDX_KS_SKIP_FINALS, L);
        iv.in_bstride = 2ll * (L + 1) * n;
        rc = launch_ntt(p, iv, batch, true, s);
    }
    if (rc || (rc = check_rows(rows, ch))) return rc;
    const u64* last_src = ntt ? prod_intt : prod_intt + (size_t)L * n;      // the special-prime rows in coefficient form
    const size_t last_stride = ntt ? n : (size_t)(L + 1) * n;
    // (one component in NTT form: the items of poly_prod are 2 (L + 1) rows apart, the INTT'd copy is compact)
    const u64* prod_for_util7 = ntt ? ks_tail_prod(c) : prod_intt;
    const unsigned prod_rows = (ntt && c.comps == 1) ? 2 * (L + 1) : L + 1;
    // (5) rounding fix of the special-prime component, per data limb (:570-598).  In NTT form the result goes to
    //     the unused tail of the prod_intt region so that step (6) can transform out of place.
    u64* util6_out = ntt ? ks_ntt_correction_rows(c) : temp_last;      // (comps <= 2: past the special rows either way)
    if (c.bgv) {
        // kernel_ski_util5_merged_step1 (:436-476): delta_j = (k mod q_j) * q_special + c mod q_j, k = -c * q_special^-1 mod t
        hipLaunchKernelGGL(bgv_delta_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s,
                           ch, p->d_mods, L, n, c.bgv->t, c.bgv->inv_special_mod_t, p->moduli[K - 1], last_src, last_stride, util6_out);
        LAUNCH_CHECK();
    } else if (ntt) {
        hipLaunchKernelGGL(ks_util6_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s,
                           ch, p->d_mods, K, L, n, last_src, last_stride, util6_out);
        LAUNCH_CHECK();
    }   // coefficient form: ks_util7_kernel forms the fix itself from the special-prime row
    // (6) back to NTT form when needed (:1033-1036)
    if (ntt && (rc = launch_ntt(p, contiguous_args(p, util6_out, temp_last, c.comps, L, 0, L, TROYN_IDX_COMPONENTWISE, 0), batch, false, s))) return rc;
    // (7) divide by the special prime and assign (:625-658; BGV: kernel_ski_util5_merged_step2 :506-538)
    if (c.bgv) {
        hipLaunchKernelGGL(bgv_finish_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s,
                           ch, p->d_mods, L, L + 1, n, prod_for_util7, temp_last, p->d_inv_last + (size_t)K * K, c.assign_method, c.dest, c.addend, c.addend_bstride);
        LAUNCH_CHECK();
    } else {
        hipLaunchKernelGGL(ks_util7_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s,
                           ch, p->d_mods, L, prod_rows, n, prod_for_util7, temp_last,
                           p->d_inv_last + (size_t)K * K, c.is_ckks, c.assign_method, c.dest, c.addend, c.addend_bstride,
                           ntt ? (const u64*)nullptr : last_src, last_stride, K);
        LAUNCH_CHECK();
    }
    return TROYN_OK;
}
// (4)-(7): divide poly_prod by the special prime and assign to dest
static int ks_tail(const KsCall& c, const KsPath& path) {
    if (path.tail == KS_TAIL_SMALL) return ks_tail_small(c);
    if (path.tail == KS_TAIL_NTT_FUSED) return ks_tail_ntt_fused(c);
    return path.tail == KS_TAIL_COEFF_FUSED ? ks_tail_coeff_fused(c) : ks_tail_unfused(c);
}

// The division of the hoisted BGV entries (bgv_hoist_kernels.hpp), NTT form, both components of `batch` items: the steps of ks_tail_unfused
// in its regions, with the special row read once per (item, component) and two coefficients per thread in both element-wise passes.
static int bgv_hoist_tail(const KsCall& c) {
    const troyn_plan* p = c.p; const unsigned L = c.L, K = p->K, n = p->n;
    const size_t batch = c.batch;
    hipStream_t s = c.s;
    u64* spec = c.ws + c.w.prod_intt;
    u64* delta = ks_ntt_correction_rows(c);            // the rest of the prod_intt region: [batch][2][L][N], where ks_tail_unfused puts its own
    u64* delta_ntt = c.ws + c.w.temp_last;
    const unsigned ch = chunks_pairs(n);
    if (int rc = check_rows(batch * 2 * L, ch)) return rc;
    // (4) the special rows in coefficient form
    if (int rc = launch_ntt(p, special_rows_args(p, ks_tail_prod(c), spec, L, 2), batch, true, s)) return rc;
    // (5) dk_j(s) for every data limb, the mod-t multiplier formed once per coefficient
    hipLaunchKernelGGL(bgv_hoist_delta_kernel, dim3((unsigned)(batch * 2 * ch)), dim3(POLY_BLOCK), 0, s,
                       ch, p->d_mods, L, n, c.bgv->t, c.bgv->inv_special_mod_t, p->moduli[K - 1], spec, delta);
    LAUNCH_CHECK();
    // (6) back to NTT form
    if (int rc = launch_ntt(p, contiguous_args(p, delta, delta_ntt, 2, L, 0, L, TROYN_IDX_COMPONENTWISE, 0), batch, false, s)) return rc;
    // (7) (X - NTT(delta)) / q_special into the destination
    const dim3 grid((unsigned)(batch * 2 * L * ch)), block(POLY_BLOCK);
    const ulonglong2* inv_k = p->d_inv_last + (size_t)K * K;
    if (c.assign_method == TROYN_ASSIGN_OVERWRITE_EXCEPT_FIRST)
        hipLaunchKernelGGL((bgv_hoist_finish_kernel<true>), grid, block, 0, s, ch, p->d_mods, L, n, ks_tail_prod(c), delta_ntt, inv_k, c.dest);
    else
        hipLaunchKernelGGL((bgv_hoist_finish_kernel<false>), grid, block, 0, s, ch, p->d_mods, L, n, ks_tail_prod(c), delta_ntt, inv_k, c.dest);
    LAUNCH_CHECK();
    return TROYN_OK;
}
// the tail of a hoisted entry on `c.batch` items: troyn_switch_key's, or the BGV division when the call carries its constants
static int hoist_tail(const KsCall& c) {
    if (c.bgv) return bgv_hoist_tail(c);
    return ks_tail(c, ks_path(c.p, c.L, c.batch, c.is_ntt_form, false));
}

static int switch_key_impl(const troyn_plan* p, unsigned L, int is_ckks, int is_ntt_form,
                           const u64* target, size_t target_bstride, const uint64_t* const* keys, int assign_method,
                           u64* dest, const u64* addend, size_t addend_bstride,
                           void* workspace, size_t workspace_bytes, size_t batch, hipStream_t s, const BgvTail* bgv = nullptr) {
    const unsigned K = p->K;
    if (K < 2) return fail(TROYN_E_INVALID, "[Evaluator::switch_key_inplace_internal] Keyswitching is not supported.");
    if (L < 1 || L > K - 1) return fail(TROYN_E_INVALID, "[Evaluator::switch_key_inplace_internal] Invalid target size.");
    if (!target || !keys || !dest || !workspace) return fail(TROYN_E_INVALID, "[Evaluator::switch_key_inplace_internal] null argument");
    if (assign_method < 0 || assign_method > 2) return fail(TROYN_E_INVALID, "[Evaluator::switch_key_inplace_internal] bad assign method");
    const KsLayout w = ks_layout(p, L, batch);
    if (workspace_bytes < w.total * sizeof(u64)) return fail(TROYN_E_WORKSPACE, "[troyn_switch_key] workspace too small");
    if (batch == 0) return TROYN_OK;
    KeyPtrs kp;
    std::memset(&kp, 0, sizeof(kp));
    for (unsigned j = 0; j < L; j++) {
        if (!keys[j]) return fail(TROYN_E_INVALID, "[Evaluator::switch_key_inplace_internal] null key pointer");
        kp.p[j] = (const u64*)keys[j];
    }
    KsCall c{p, L, is_ckks, is_ntt_form != 0, target, target_bstride, assign_method, dest, addend, addend_bstride,
             (u64*)workspace, w, batch, s, bgv, target, target_bstride};
    const KsPath path = ks_path(p, L, batch, c.is_ntt_form, bgv != nullptr);
    if (int rc = ks_digits(c)) return rc;
    if (int rc = ks_inner_product(c, kp, path)) return rc;
    return ks_tail(c, path);
}

extern "C" int troyn_switch_key(const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form,
                                const uint64_t* target, const uint64_t* const* keys, int assign_method,
                                uint64_t* destination, void* workspace, size_t workspace_bytes,
                                size_t batch, troyn_stream_t stream) {
    select_device(plan);
    if (!plan) return fail(TROYN_E_INVALID, "[troyn_switch_key] null plan");
    return switch_key_impl(plan, L, is_ckks, is_ntt_form, (const u64*)target, (size_t)L * plan->n, keys, assign_method,
                           (u64*)destination, nullptr, 0, workspace, workspace_bytes, batch, (hipStream_t)stream);
}

extern "C" int troyn_relinearize(const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form,
                                 const uint64_t* ct3, const uint64_t* const* keys, uint64_t* out2,
                                 void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream) {
    select_device(plan);
    if (!plan || !ct3) return fail(TROYN_E_INVALID, "[Evaluator::relinearize_inplace_internal] null argument");
    const size_t pc = (size_t)L * plan->n;
    // relinearize_internal (evaluator_keyswitching.cu:119-144): switch_key(target = c2, Overwrite) then += (c0, c1)
    return switch_key_impl(plan, L, is_ckks, is_ntt_form, (const u64*)ct3 + 2 * pc, 3 * pc, keys, TROYN_ASSIGN_OVERWRITE,
                           (u64*)out2, (const u64*)ct3, 3 * pc, workspace, workspace_bytes, batch, (hipStream_t)stream);
}

// ---- hoisted rotations (an addition to the reference's surface; include/troyn.h, hoist_kernels.hpp) ----
// One decomposition (ks_digits + ks_transform_digits) serves every term; hoist_mac_kernel forms poly_prod per slot (many: one slot per
// term, sum: one slot), hoist_c0_kernel the permuted c0, and ks_tail runs unchanged on slots * batch items.
struct HoistLayout { KsLayout ks; size_t table; };

// `slots` results per item of the batch (many: one per term, sum: one, weighted sums: the caller's count)
static HoistLayout hoist_layout(const troyn_plan* p, unsigned L, size_t terms, size_t batch, size_t slots) {
    const size_t n = p->n, items = slots * batch;
    HoistLayout h;
    size_t off = 0;
    h.ks.target_intt = off; off += batch * L * n;
    h.ks.temp_ntt = off;    off += batch * (size_t)(L + 1) * L * n;
    h.ks.poly_prod = off;   off += items * 2 * (size_t)(L + 1) * n;
    h.ks.prod_intt = off;   off += items * 2 * (size_t)(L + 1) * n;
    h.ks.temp_last = off;   off += items * 2 * (size_t)L * n;
    h.ks.keys_f64 = h.ks.split = h.ks.keys_quo = off;      // the inner products of troyn_switch_key do not run here
    h.table = off;          off += (terms * (L + 2) + 1) & ~(size_t)1;      // key pointers [terms][L], elements [terms], inverse elements [terms]
    h.ks.total = off;
    return h;
}

extern "C" size_t troyn_apply_galois_hoisted_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t terms, size_t batch, int sum) {
    if (!plan) return 0;
    return hoist_layout(plan, L, terms, batch, sum ? 1 : terms).ks.total * sizeof(u64);
}

// what every hoisted entry checks before it looks at the batch: the plan, the level, the element and key tables.  The identity element
// (no key: its L entries are not looked at) is the weighted entry's alone.
static int hoist_check_tables(const char* P, const troyn_plan* p, unsigned L, const uint64_t* galois_elements, const uint64_t* const* keys,
                              size_t terms, bool allow_identity) {
    if (!p) return fail(TROYN_E_INVALID, std::string(P) + " null plan");
    const unsigned K = p->K, n = p->n;
    if (K < 2) return fail(TROYN_E_INVALID, std::string(P) + " Keyswitching is not supported.");
    if (L < 1 || L > K - 1) return fail(TROYN_E_INVALID, std::string(P) + " Invalid target size.");
    if (terms == 0) return fail(TROYN_E_INVALID, std::string(P) + " no terms");
    if (!galois_elements || !keys) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    for (size_t t = 0; t < terms; t++) {
        const uint64_t g = galois_elements[t];
        if ((g & 1) == 0 || g >= 2ull * n || (g == 1 && !allow_identity)) return fail(TROYN_E_INVALID, std::string(P) + " Galois element is not valid.");
        if (g == 1) continue;
        for (unsigned j = 0; j < L; j++)
            if (!keys[t * L + j] || ((uintptr_t)keys[t * L + j] & 15)) return fail(TROYN_E_INVALID, std::string(P) + " null or misaligned key pointer");
    }
    return TROYN_OK;
}
// the buffers of a non-empty batch: `out` holds `items` ciphertexts and may not overlap the `batch` ciphertexts of `ct`
static int hoist_check_buffers(const char* P, const troyn_plan* p, unsigned L, const u64* ct, const u64* out, const void* workspace,
                               size_t batch, size_t items) {
    if (!ct || !out || !workspace) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (((uintptr_t)ct | (uintptr_t)out | (uintptr_t)workspace) & 15) return fail(TROYN_E_INVALID, std::string(P) + " misaligned pointer");
    const size_t ct_words = (size_t)2 * L * p->n;
    if ((uintptr_t)out < (uintptr_t)(ct + batch * ct_words) && (uintptr_t)ct < (uintptr_t)(out + items * ct_words))
        return fail(TROYN_E_INVALID, std::string(P) + " out overlaps ct");
    return TROYN_OK;
}
// the host tables of one call, [terms][L] key pointers, the elements, their inverses modulo 2N, followed by `extra`: one upload
static int hoist_upload_tables(const troyn_plan* p, unsigned L, const uint64_t* galois_elements, const uint64_t* const* keys, size_t terms,
                               const std::vector<u64>& extra, u64* dev, hipStream_t s) {
    std::vector<u64> table(terms * (L + 2));
    for (size_t t = 0; t < terms; t++) {
        const u64 g = galois_elements[t];
        for (unsigned j = 0; j < L; j++) table[t * L + j] = g == 1 ? 0 : (u64)(uintptr_t)keys[t * L + j];
        u64 inv = g;                                   // g * g = 1 (mod 8); every Newton step doubles the number of correct low bits
        for (int i = 0; i < 5; i++) inv *= 2 - g * inv;
        table[terms * L + t] = g;
        table[terms * (L + 1) + t] = inv & (2ull * p->n - 1);
    }
    table.insert(table.end(), extra.begin(), extra.end());
    return upload_host_table(s, dev, table.data(), table.size() * sizeof(u64));
}
// (1) + (2): c1 in coefficient form, then its L digits under every key modulus, once.  `dc` is also the call the tail later runs with (on
// slots * batch items); skip_diag: the transform left the diagonal blocks to the consumer.
static int hoist_decompose(KsCall& dc, bool& skip_diag) {
    if (int rc = ks_digits(dc)) return rc;
    skip_diag = dc.is_ntt_form && dc.p->log_n >= 10;      // as ks_path's `fused`
    return ks_transform_digits(dc, skip_diag);
}

static int apply_galois_hoisted(const char* P, const troyn_plan* p, unsigned L, int is_ckks, int is_ntt_form, const u64* ct,
                                const uint64_t* galois_elements, const uint64_t* const* keys, size_t terms, u64* out,
                                void* workspace, size_t workspace_bytes, size_t batch, hipStream_t s, bool sum, const BgvTail* bgv = nullptr) {
    if (int rc = hoist_check_tables(P, p, L, galois_elements, keys, terms, false)) return rc;
    const unsigned K = p->K, n = p->n;
    if (batch == 0) return TROYN_OK;      // nothing to do: neither ct, out nor the workspace is looked at
    const size_t slots = sum ? 1 : terms, items = slots * batch, ct_words = (size_t)2 * L * n;
    if (int rc = hoist_check_buffers(P, p, L, ct, out, workspace, batch, items)) return rc;
    const HoistLayout h = hoist_layout(p, L, terms, batch, slots);
    if (workspace_bytes < h.ks.total * sizeof(u64)) return fail(TROYN_E_WORKSPACE, std::string(P) + " workspace too small");
    u64* ws = (u64*)workspace;
    // the tables are read before the call returns
    if (int rc = hoist_upload_tables(p, L, galois_elements, keys, terms, {}, ws + h.table, s)) return rc;
    const u64* c1 = ct + (size_t)L * n;
    KsCall dc{p, L, is_ckks, is_ntt_form != 0, c1, ct_words, TROYN_ASSIGN_OVERWRITE_EXCEPT_FIRST, out, nullptr, 0,
              ws, h.ks, batch, s, bgv, c1, ct_words};
    bool skip_diag = false;
    if (int rc = hoist_decompose(dc, skip_diag)) return rc;
    HoistArgs a;
    std::memset(&a, 0, sizeof(a));
    a.mods = p->d_mods; a.K = K; a.L = L; a.log_n = p->log_n; a.batch = (unsigned)batch;
    a.terms_per_slot = (unsigned)(sum ? terms : 1); a.is_ntt_form = dc.is_ntt_form ? 1 : 0;
    a.ct = ct; a.digits_ntt = ws + h.ks.temp_ntt; a.diag_from_ct = skip_diag ? 1 : 0;
    a.keys = reinterpret_cast<const u64* const*>(ws + h.table);
    a.elements = ws + h.table + terms * L; a.inv_elements = a.elements + terms;
    a.poly_prod = ws + h.ks.poly_prod; a.dest = out;
    if (batch > 0xffffffffull || terms > 0xffffffffull) return fail(TROYN_E_INVALID, std::string(P) + " batch too large for one launch");
    // (3) the permuted c0 (summed over the terms in the sum form) into component 0 of the destination
    {
        const unsigned ch = chunks_single(n);
        const size_t rows = items * L;
        if (int rc = check_rows(rows, ch)) return rc;
        hipLaunchKernelGGL(hoist_c0_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s, ch, a);
        LAUNCH_CHECK();
    }
    // (4) <permuted digits, keys>: a workgroup carries up to four items of the batch through the same key words
    {
        const unsigned ib = batch >= 4 ? 4u : batch >= 2 ? 2u : 1u;
        a.groups = (unsigned)((batch + ib - 1) / ib);
        const unsigned ch = chunks_pairs(n);
        const size_t rows = slots * a.groups * (size_t)(L + 1);
        if (int rc = check_rows(rows, ch)) return rc;
        TimerScope ts(TROYN_TIMER_KS_INNER_PRODUCT, s);
        const dim3 grid((unsigned)(rows * ch)), block(POLY_BLOCK);
        if (ib == 4) hipLaunchKernelGGL((hoist_mac_kernel<4>), grid, block, 0, s, ch, a);
        else if (ib == 2) hipLaunchKernelGGL((hoist_mac_kernel<2>), grid, block, 0, s, ch, a);
        else hipLaunchKernelGGL((hoist_mac_kernel<1>), grid, block, 0, s, ch, a);
        LAUNCH_CHECK();
    }
    // (5) the tail of troyn_switch_key on slots * batch items: dest[.][0] += result_0, dest[.][1] = result_1
    KsCall tc = dc;
    tc.batch = items;
    return hoist_tail(tc);
}

extern "C" int troyn_apply_galois_many(const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form, const uint64_t* ct,
                                       const uint64_t* galois_elements, const uint64_t* const* keys, size_t terms, uint64_t* out,
                                       void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream) {
    select_device(plan);
    return apply_galois_hoisted("[troyn_apply_galois_many]", plan, L, is_ckks, is_ntt_form, (const u64*)ct, galois_elements, keys, terms,
                                (u64*)out, workspace, workspace_bytes, batch, (hipStream_t)stream, false);
}
extern "C" int troyn_apply_galois_sum(const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form, const uint64_t* ct,
                                      const uint64_t* galois_elements, const uint64_t* const* keys, size_t terms, uint64_t* out,
                                      void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream) {
    select_device(plan);
    return apply_galois_hoisted("[troyn_apply_galois_sum]", plan, L, is_ckks, is_ntt_form, (const u64*)ct, galois_elements, keys, terms,
                                (u64*)out, workspace, workspace_bytes, batch, (hipStream_t)stream, true);
}

// ---- plaintext-weighted hoisted rotations (an addition; include/troyn.h, hoist_weighted_kernel) ----
// out[s] = SUM_t w_{s,t} (.) sigma_{g_t}(ct): the weight enters between the per-term reduction and the sum, on the extended basis, and the
// unkeyed contributions are injected there scaled by q_special -- so ONE tail per slot (TROYN_ASSIGN_OVERWRITE) finishes both components.
struct WeightedLayout { HoistLayout h; size_t weights, special_mod, c0_ntt, total; };

static WeightedLayout weighted_layout(const troyn_plan* p, unsigned L, size_t terms, size_t slots, size_t batch, bool is_ntt_form) {
    WeightedLayout w;
    w.h = hoist_layout(p, L, terms, batch, slots);
    size_t off = w.h.table + terms * (L + 2);           // the extra tables follow the hoisted ones: one upload
    w.weights = off;     off += slots * terms;
    w.special_mod = off; off += L;
    off = (off + 1) & ~(size_t)1;
    w.c0_ntt = off;      off += is_ntt_form ? 0 : batch * L * (size_t)p->n;      // coefficient form: the forward transform of c0
    w.total = off;
    return w;
}

extern "C" size_t troyn_apply_galois_weighted_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t terms, size_t slots, size_t batch,
                                                              int is_ntt_form) {
    if (!plan) return 0;
    return weighted_layout(plan, L, terms, slots, batch, is_ntt_form != 0).total * sizeof(u64);
}

// the entry's work.  layout: the caller's own placement of the same regions (null: weighted_layout); finish = false stops after the
// extended-basis sums, poly_prod [slots][batch][2][L+1][N] in NTT form, and leaves `out` unwritten (the double-hoisted BSGS transform)
static int weighted_sums_impl(const char* P, const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form, const uint64_t* ct_,
                              const uint64_t* galois_elements, const uint64_t* const* keys, size_t terms,
                              const uint64_t* const* weights, size_t slots, uint64_t* out_,
                              void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream,
                              const WeightedLayout* layout, bool finish, const BgvTail* bgv = nullptr) {
    const troyn_plan* p = plan;
    const u64* ct = (const u64*)ct_;
    u64* out = (u64*)out_;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = hoist_check_tables(P, p, L, galois_elements, keys, terms, true)) return rc;
    if (slots == 0) return fail(TROYN_E_INVALID, std::string(P) + " no slots");
    if (!weights) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    for (size_t sl = 0; sl < slots; sl++) {
        bool any = false;
        for (size_t t = 0; t < terms; t++) {
            const uint64_t* w = weights[sl * terms + t];
            if ((uintptr_t)w & 15) return fail(TROYN_E_INVALID, std::string(P) + " misaligned weight pointer");
            any = any || w;
        }
        if (!any) return fail(TROYN_E_INVALID, std::string(P) + " a slot has no weight");
    }
    const unsigned K = p->K, n = p->n;
    if (batch == 0) return TROYN_OK;      // nothing to do: neither ct, out nor the workspace is looked at
    const size_t items = slots * batch, ct_words = (size_t)2 * L * n;
    // (finish = false writes no `out`: the caller has checked its own buffers)
    if (finish) if (int rc = hoist_check_buffers(P, p, L, ct, out, workspace, batch, items)) return rc;
    const bool ntt = is_ntt_form != 0;
    const WeightedLayout w = layout ? *layout : weighted_layout(p, L, terms, slots, batch, ntt);
    if (workspace_bytes < w.total * sizeof(u64)) return fail(TROYN_E_WORKSPACE, std::string(P) + " workspace too small");
    if (batch > 0xffffffffull || terms > 0xffffffffull || slots > 0xffffffffull) return fail(TROYN_E_INVALID, std::string(P) + " batch too large for one launch");
    u64* ws = (u64*)workspace;
    // the tables are read before the call returns: the hoisted tables, then [slots][terms] weight pointers and q_special mod q_l
    std::vector<u64> extra(slots * terms + L);
    for (size_t i = 0; i < slots * terms; i++) extra[i] = (u64)(uintptr_t)weights[i];
    for (unsigned l = 0; l < L; l++) extra[slots * terms + l] = p->moduli[K - 1] % p->moduli[l];
    if (int rc = hoist_upload_tables(p, L, galois_elements, keys, terms, extra, ws + w.h.table, s)) return rc;
    const u64* c1 = ct + (size_t)L * n;
    KsCall dc{p, L, is_ckks, ntt, c1, ct_words, TROYN_ASSIGN_OVERWRITE, out, nullptr, 0,
              ws, w.h.ks, batch, s, bgv, c1, ct_words};
    bool skip_diag = false;
    if (int rc = hoist_decompose(dc, skip_diag)) return rc;
    HoistWeightedArgs a;
    std::memset(&a, 0, sizeof(a));
    a.mods = p->d_mods; a.K = K; a.L = L; a.log_n = p->log_n; a.batch = (unsigned)batch; a.terms = (unsigned)terms;
    a.digits_ntt = ws + w.h.ks.temp_ntt; a.diag_from_c1 = skip_diag ? 1 : 0;
    if (ntt) {
        a.c0_ntt = ct; a.c0_bstride = ct_words;
        a.c1_ntt = c1; a.c1_bstride = ct_words; a.c1_lstride = n;
    } else {
        // the NTT-form limbs of c0: one forward transform; those of c1 are the diagonal blocks D[l][l], present in coefficient form
        NttArgs f = contiguous_args(p, ct, ws + w.c0_ntt, 1, L, 0, L, TROYN_IDX_COMPONENTWISE, 0);
        f.in_bstride = (long long)ct_words;
        if (int rc = launch_ntt(p, f, batch, false, s)) return rc;
        a.c0_ntt = ws + w.c0_ntt; a.c0_bstride = (size_t)L * n;
        a.c1_ntt = a.digits_ntt; a.c1_bstride = (size_t)(L + 1) * L * n; a.c1_lstride = (size_t)(L + 1) * n;
    }
    a.keys = reinterpret_cast<const u64* const*>(ws + w.h.table);
    a.elements = ws + w.h.table + terms * L;
    a.weights = reinterpret_cast<const u64* const*>(ws + w.weights);
    a.special_mod = ws + w.special_mod;
    a.poly_prod = ws + w.h.ks.poly_prod;
    // <permuted digits, keys>, the weight, the sum over the slot's terms and the scaled unkeyed contributions in one launch
    {
        const unsigned ib = batch >= 4 ? 4u : batch >= 2 ? 2u : 1u;
        a.groups = (unsigned)((batch + ib - 1) / ib);
        const unsigned ch = chunks_pairs(n);
        const size_t rows = slots * a.groups * (size_t)(L + 1);
        if (int rc = check_rows(rows, ch)) return rc;
        TimerScope ts(TROYN_TIMER_KS_INNER_PRODUCT, s);
        const dim3 grid((unsigned)(rows * ch)), block(POLY_BLOCK);
        if (ib == 4) hipLaunchKernelGGL((hoist_weighted_kernel<4>), grid, block, 0, s, ch, a);
        else if (ib == 2) hipLaunchKernelGGL((hoist_weighted_kernel<2>), grid, block, 0, s, ch, a);
        else hipLaunchKernelGGL((hoist_weighted_kernel<1>), grid, block, 0, s, ch, a);
        LAUNCH_CHECK();
    }
    if (!finish) return TROYN_OK;
    // the tail of troyn_switch_key on slots * batch items, both components overwritten
    KsCall tc = dc;
    tc.batch = items;
    return hoist_tail(tc);
}

extern "C" int troyn_apply_galois_weighted_sums(const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form, const uint64_t* ct,
                                                const uint64_t* galois_elements, const uint64_t* const* keys, size_t terms,
                                                const uint64_t* const* weights, size_t slots, uint64_t* out,
                                                void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream) {
    select_device(plan);
    return weighted_sums_impl("[troyn_apply_galois_weighted_sums]", plan, L, is_ckks, is_ntt_form, ct, galois_elements, keys, terms, weights, slots,
                              out, workspace, workspace_bytes, batch, stream, nullptr, true);
}

// ---- the sum of key-switched automorphisms of DIFFERENT ciphertexts (an addition; include/troyn.h, hoist_each_kernel) ----
// out = SUM_t sigma_{g_t}(cts[t]): the decomposition runs with terms * batch as its batch, hoist_each_kernel sums the terms on the extended
// basis (the unkeyed contributions scaled by q_special, as in the weighted entry), ONE tail on `batch` items finishes both components.  The
// digits of at most TROYN_HOIST_EACH_GROUP terms are resident at once; later groups add into poly_prod.
struct EachLayout { KsLayout ks; size_t table, c0_ntt, total; };

static EachLayout each_layout(const troyn_plan* p, unsigned L, size_t terms, size_t batch, bool is_ntt_form) {
    const size_t n = p->n, resident = std::min<size_t>(terms, TROYN_HOIST_EACH_GROUP) * batch;
    EachLayout e;
    size_t off = 0;
    e.ks.target_intt = off; off += resident * L * n;
    e.ks.temp_ntt = off;    off += resident * (size_t)(L + 1) * L * n;
    e.ks.poly_prod = off;   off += batch * 2 * (size_t)(L + 1) * n;
    e.ks.prod_intt = off;   off += batch * 2 * (size_t)(L + 1) * n;
    e.ks.temp_last = off;   off += batch * 2 * (size_t)L * n;
    e.ks.keys_f64 = e.ks.split = e.ks.keys_quo = off;      // the inner products of troyn_switch_key do not run here
    e.table = off;          off += std::min<size_t>(terms, TROYN_HOIST_EACH_GROUP) * (L + 2) + L;      // one group's hoisted tables, then q_special mod q_l
    off = (off + 1) & ~(size_t)1;
    e.c0_ntt = off;         off += is_ntt_form ? 0 : resident * L * n;      // coefficient form: the forward transform of the group's c0
    e.total = e.ks.total = off;
    return e;
}

extern "C" size_t troyn_apply_galois_sum_each_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t terms, size_t batch, int is_ntt_form) {
    if (!plan) return 0;
    return each_layout(plan, L, terms, batch, is_ntt_form != 0).total * sizeof(u64);
}

// the entry's work once the element and key tables have passed hoist_check_tables
static int apply_galois_sum_each(const char* P, const troyn_plan* p, unsigned L, int is_ckks, int is_ntt_form, const u64* cts,
                                 const uint64_t* galois_elements, const uint64_t* const* keys, size_t terms, u64* out,
                                 void* workspace, size_t workspace_bytes, size_t batch, hipStream_t s, const BgvTail* bgv = nullptr) {
    const unsigned K = p->K, n = p->n;
    if (batch == 0) return TROYN_OK;      // nothing to do: neither cts, out nor the workspace is looked at
    const size_t ct_words = (size_t)2 * L * n;
    if (terms > 0xffffffffull || batch > 0xffffffffull || terms * batch > 0xffffffffull)
        return fail(TROYN_E_INVALID, std::string(P) + " batch too large for one launch");
    if (int rc = hoist_check_buffers(P, p, L, cts, out, workspace, terms * batch, batch)) return rc;
    const bool ntt = is_ntt_form != 0;
    const EachLayout e = each_layout(p, L, terms, batch, ntt);
    if (workspace_bytes < e.total * sizeof(u64)) return fail(TROYN_E_WORKSPACE, std::string(P) + " workspace too small");
    u64* ws = (u64*)workspace;
    std::vector<u64> special(L);
    for (unsigned l = 0; l < L; l++) special[l] = p->moduli[K - 1] % p->moduli[l];
    const unsigned ib = batch >= 4 ? 4u : batch >= 2 ? 2u : 1u;
    const unsigned ch = chunks_pairs(n);
    const size_t groups = (batch + ib - 1) / ib, rows = groups * (size_t)(L + 1);
    if (int rc = check_rows(rows, ch)) return rc;
    for (size_t t0 = 0; t0 < terms; t0 += TROYN_HOIST_EACH_GROUP) {
        const size_t gt = std::min<size_t>(terms - t0, TROYN_HOIST_EACH_GROUP);
        const u64* ct = cts + t0 * batch * ct_words;      // the group's ciphertexts: gt * batch items, ct_words apart
        // the tables are read before the call returns (a group's upload waits on the stream for the launch that read the last one)
        if (int rc = hoist_upload_tables(p, L, galois_elements + t0, keys + t0 * L, gt, special, ws + e.table, s)) return rc;
        const u64* c1 = ct + (size_t)L * n;
        KsCall dc{p, L, is_ckks, ntt, c1, ct_words, TROYN_ASSIGN_OVERWRITE, out, nullptr, 0,
                  ws, e.ks, gt * batch, s, nullptr, c1, ct_words};
        bool skip_diag = false;
        if (int rc = hoist_decompose(dc, skip_diag)) return rc;
        HoistEachArgs a;
        std::memset(&a, 0, sizeof(a));
        a.mods = p->d_mods; a.K = K; a.L = L; a.log_n = p->log_n; a.batch = (unsigned)batch; a.groups = (unsigned)groups;
        a.terms = (unsigned)gt; a.accumulate = t0 ? 1 : 0;
        a.digits_ntt = ws + e.ks.temp_ntt; a.diag_from_c1 = skip_diag ? 1 : 0;
        if (ntt) {
            a.c0_ntt = ct; a.c0_bstride = ct_words;
            a.c1_ntt = c1; a.c1_bstride = ct_words; a.c1_lstride = n;
        } else {
            // BFV: the unkeyed contributions are injected after ONE forward transform of the group's c0 into the workspace; the NTT-form limbs
            // of c1 (identity terms) are the diagonal blocks D[l][l], present in coefficient form
            NttArgs f = contiguous_args(p, ct, ws + e.c0_ntt, 1, L, 0, L, TROYN_IDX_COMPONENTWISE, 0);
            f.in_bstride = (long long)ct_words;
            if (int rc = launch_ntt(p, f, gt * batch, false, s)) return rc;
            a.c0_ntt = ws + e.c0_ntt; a.c0_bstride = (size_t)L * n;
            a.c1_ntt = a.digits_ntt; a.c1_bstride = (size_t)(L + 1) * L * n; a.c1_lstride = (size_t)(L + 1) * n;
        }
        a.keys = reinterpret_cast<const u64* const*>(ws + e.table);
        a.elements = ws + e.table + gt * L;
        a.special_mod = ws + e.table + gt * (L + 2);
        a.poly_prod = ws + e.ks.poly_prod;
        {
            TimerScope ts(TROYN_TIMER_KS_INNER_PRODUCT, s);
            const dim3 grid((unsigned)(rows * ch)), block(POLY_BLOCK);
            if (ib == 4) hipLaunchKernelGGL((hoist_each_kernel<4>), grid, block, 0, s, ch, a);
            else if (ib == 2) hipLaunchKernelGGL((hoist_each_kernel<2>), grid, block, 0, s, ch, a);
            else hipLaunchKernelGGL((hoist_each_kernel<1>), grid, block, 0, s, ch, a);
            LAUNCH_CHECK();
        }
    }
    // the tail of troyn_switch_key on `batch` items, both components overwritten
    const u64* c1 = cts + (size_t)L * n;
    KsCall tc{p, L, is_ckks, ntt, c1, ct_words, TROYN_ASSIGN_OVERWRITE, out, nullptr, 0,
              ws, e.ks, batch, s, bgv, c1, ct_words};
    return hoist_tail(tc);
}

extern "C" int troyn_apply_galois_sum_each(const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form, const uint64_t* cts,
                                           const uint64_t* galois_elements, const uint64_t* const* keys, size_t terms, uint64_t* out,
                                           void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream) {
    select_device(plan);
    const char* P = "[troyn_apply_galois_sum_each]";
    if (int rc = hoist_check_tables(P, plan, L, galois_elements, keys, terms, true)) return rc;
    return apply_galois_sum_each(P, plan, L, is_ckks, is_ntt_form, (const u64*)cts, galois_elements, keys, terms, (u64*)out,
                                 workspace, workspace_bytes, batch, (hipStream_t)stream);
}

// ---- baby-step/giant-step linear transform (an addition; include/troyn.h): the weighted sums over the baby steps, one per giant step, into
// the workspace, then the sum of their giant-step automorphisms with ONE division ----
struct BsgsLayout { size_t inner, stage, stage_words, total; };

static BsgsLayout bsgs_layout(const troyn_plan* p, unsigned L, size_t babies, size_t giants, size_t batch, bool is_ntt_form) {
    BsgsLayout b;
    b.inner = 0;                                                       // [giants][batch][2][L][N], never visible to the caller
    b.stage = giants * batch * 2 * (size_t)L * p->n;                   // one workspace, used by the stages one after the other
    b.stage_words = std::max(weighted_layout(p, L, babies, giants, batch, is_ntt_form).total, each_layout(p, L, giants, batch, is_ntt_form).total);
    b.total = b.stage + b.stage_words;
    return b;
}

extern "C" size_t troyn_linear_transform_bsgs_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t babies, size_t giants, size_t batch,
                                                              int is_ntt_form) {
    if (!plan) return 0;
    return bsgs_layout(plan, L, babies, giants, batch, is_ntt_form != 0).total * sizeof(u64);
}

// what both BSGS entries check before they look at the batch: the two element and key tables and the weight table
static int bsgs_check_tables(const char* P, const troyn_plan* p, unsigned L, const uint64_t* baby_elements, const uint64_t* const* baby_keys, size_t babies,
                             const uint64_t* giant_elements, const uint64_t* const* giant_keys, size_t giants, const uint64_t* const* weights) {
    if (int rc = hoist_check_tables(P, p, L, baby_elements, baby_keys, babies, true)) return rc;
    if (int rc = hoist_check_tables(P, p, L, giant_elements, giant_keys, giants, true)) return rc;
    if (!weights) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    for (size_t g = 0; g < giants; g++) {
        bool any = false;
        for (size_t b = 0; b < babies; b++) {
            const uint64_t* w = weights[g * babies + b];
            if ((uintptr_t)w & 15) return fail(TROYN_E_INVALID, std::string(P) + " misaligned weight pointer");
            any = any || w;
        }
        if (!any) return fail(TROYN_E_INVALID, std::string(P) + " a giant step has no weight");
    }
    return TROYN_OK;
}

// the driver of both BSGS entries; P names the entry, PW its inner stage
static int linear_transform_bsgs_impl(const char* P, const char* PW, const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form, const uint64_t* ct_,
                                      const uint64_t* baby_elements, const uint64_t* const* baby_keys, size_t babies,
                                      const uint64_t* giant_elements, const uint64_t* const* giant_keys, size_t giants,
                                      const uint64_t* const* weights, uint64_t* out_,
                                      void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream, const BgvTail* bgv) {
    const troyn_plan* p = plan;
    const u64* ct = (const u64*)ct_;
    u64* out = (u64*)out_;
    if (int rc = bsgs_check_tables(P, p, L, baby_elements, baby_keys, babies, giant_elements, giant_keys, giants, weights)) return rc;
    if (batch == 0) return TROYN_OK;      // nothing to do: neither ct, out nor the workspace is looked at
    if (int rc = hoist_check_buffers(P, p, L, ct, out, workspace, batch, batch)) return rc;
    const BsgsLayout b = bsgs_layout(p, L, babies, giants, batch, is_ntt_form != 0);
    if (workspace_bytes < b.total * sizeof(u64)) return fail(TROYN_E_WORKSPACE, std::string(P) + " workspace too small");
    u64* ws = (u64*)workspace;
    u64* inner = ws + b.inner;
    // stage 1: one decomposition of ct, `giants` divisions -- inner[g] = SUM_b w_{g,b} (.) sigma_{B_b}(ct)
    if (int rc = weighted_sums_impl(PW, plan, L, is_ckks, is_ntt_form, ct_, baby_elements, baby_keys, babies, weights, giants,
                                    (uint64_t*)inner, ws + b.stage, b.stage_words * sizeof(u64), batch, stream, nullptr, true, bgv)) return rc;
    // stage 2: out = SUM_g sigma_{G_g}(inner[g]), ONE division
    return apply_galois_sum_each(P, p, L, is_ckks, is_ntt_form, inner, giant_elements, giant_keys, giants, out,
                                 ws + b.stage, b.stage_words * sizeof(u64), batch, (hipStream_t)stream, bgv);
}

extern "C" int troyn_linear_transform_bsgs(const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form, const uint64_t* ct_,
                                           const uint64_t* baby_elements, const uint64_t* const* baby_keys, size_t babies,
                                           const uint64_t* giant_elements, const uint64_t* const* giant_keys, size_t giants,
                                           const uint64_t* const* weights, uint64_t* out_,
                                           void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream) {
    select_device(plan);
    return linear_transform_bsgs_impl("[troyn_linear_transform_bsgs]", "[troyn_apply_galois_weighted_sums]", plan, L, is_ckks, is_ntt_form, ct_,
                                      baby_elements, baby_keys, babies, giant_elements, giant_keys, giants, weights, out_,
                                      workspace, workspace_bytes, batch, stream, nullptr);
}

// ---- double-hoisted BSGS linear transform (an addition; include/troyn.h, hoist_double_kernel): the inner sums stay on the extended basis in
// the workspace; per giant step with G != 1 only component 1 is divided (it is what the giant key decomposes), component 0 goes through the
// giant automorphism on the extended basis into the outer sum; an identity giant step adds both components undivided.  ONE division of both
// components ends the transform ----
struct DoubleLayout { WeightedLayout inner; size_t v, y, total; };

// Regions of one group of min(giants, TROYN_HOIST_EACH_GROUP) giant steps serve the inner stage (which needs `batch` items of them) and every
// group of the outer stage; only X, the inner results [giants][batch][2][L+1][N], grows with `giants`.
static DoubleLayout double_layout(const troyn_plan* p, unsigned L, size_t babies, size_t giants, size_t batch, bool is_ntt_form) {
    const size_t n = p->n, group = std::min<size_t>(giants, TROYN_HOIST_EACH_GROUP), resident = group * batch;
    DoubleLayout d;
    KsLayout& k = d.inner.h.ks;
    size_t off = 0;
    k.target_intt = off; off += resident * L * n;
    k.temp_ntt = off;    off += resident * (size_t)(L + 1) * L * n;
    k.poly_prod = off;   off += giants * batch * 2 * (size_t)(L + 1) * n;      // X
    k.prod_intt = off;   off += resident * 2 * (size_t)(L + 1) * n;            // the tails' own rows: a group's inner divisions, then the final one
    k.temp_last = off;   off += resident * 2 * (size_t)L * n;
    k.keys_f64 = k.split = k.keys_quo = off;      // the inner products of troyn_switch_key do not run here
    d.v = off;           off += resident * L * n;                              // v^(g) of one group [group][batch][L][N]
    d.y = off;           off += batch * 2 * (size_t)(L + 1) * n;               // Y, the outer sum
    // the inner stage's tables (hoisted tables, weight pointers, q_special mod q_l: one upload), later one group's hoisted tables in their place
    d.inner.h.table = off;
    d.inner.weights = off + babies * (L + 2);
    d.inner.special_mod = d.inner.weights + giants * babies;
    off += std::max(babies * (L + 2) + giants * babies + L, group * (L + 2));
    off = (off + 1) & ~(size_t)1;
    d.inner.c0_ntt = off; off += is_ntt_form ? 0 : batch * L * n;              // coefficient form: the inner stage's forward transform of c0
    d.total = d.inner.total = k.total = off;
    return d;
}

extern "C" size_t troyn_linear_transform_bsgs_double_hoisted_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t babies, size_t giants,
                                                                             size_t batch, int is_ntt_form) {
    if (!plan) return 0;
    return double_layout(plan, L, babies, giants, batch, is_ntt_form != 0).total * sizeof(u64);
}

extern "C" int troyn_linear_transform_bsgs_double_hoisted(const troyn_plan* plan, uint32_t L, int is_ckks, int is_ntt_form, const uint64_t* ct_,
                                                          const uint64_t* baby_elements, const uint64_t* const* baby_keys, size_t babies,
                                                          const uint64_t* giant_elements, const uint64_t* const* giant_keys, size_t giants,
                                                          const uint64_t* const* weights, uint64_t* out_,
                                                          void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream) {
    select_device(plan);
    const char* P = "[troyn_linear_transform_bsgs_double_hoisted]";
    const troyn_plan* p = plan;
    const u64* ct = (const u64*)ct_;
    u64* out = (u64*)out_;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = bsgs_check_tables(P, p, L, baby_elements, baby_keys, babies, giant_elements, giant_keys, giants, weights)) return rc;
    if (batch == 0) return TROYN_OK;      // nothing to do: neither ct, out nor the workspace is looked at
    if (int rc = hoist_check_buffers(P, p, L, ct, out, workspace, batch, batch)) return rc;
    const bool ntt = is_ntt_form != 0;
    const DoubleLayout d = double_layout(p, L, babies, giants, batch, ntt);
    if (workspace_bytes < d.total * sizeof(u64)) return fail(TROYN_E_WORKSPACE, std::string(P) + " workspace too small");
    if (giants > 0xffffffffull || batch > 0xffffffffull || giants * batch > 0xffffffffull)
        return fail(TROYN_E_INVALID, std::string(P) + " batch too large for one launch");
    const unsigned K = p->K, n = p->n;
    u64* ws = (u64*)workspace;
    // stage 1: one decomposition of ct; X^(g) = the weighted sums over the baby steps on the extended basis, NOT divided
    if (int rc = weighted_sums_impl(P, plan, L, is_ckks, is_ntt_form, ct_, baby_elements, baby_keys, babies, weights, giants, out_,
                                    workspace, workspace_bytes, batch, stream, &d.inner, false)) return rc;
    const KsLayout& k = d.inner.h.ks;
    const size_t x_item = 2 * (size_t)(L + 1) * n, v_item = (size_t)L * n, digit_item = (size_t)(L + 1) * L * n, ct_words = (size_t)2 * L * n;
    const unsigned ib = batch >= 4 ? 4u : batch >= 2 ? 2u : 1u;
    const unsigned ch = chunks_pairs(n);
    const size_t groups = (batch + ib - 1) / ib, rows = groups * (size_t)(L + 1);
    if (int rc = check_rows(rows, ch)) return rc;
    // stage 2, per group of giant steps: v^(g) = component 1 of X^(g) divided (G != 1 only), its digits, then the sum into Y
    for (size_t t0 = 0; t0 < giants; t0 += TROYN_HOIST_EACH_GROUP) {
        const size_t gt = std::min<size_t>(giants - t0, TROYN_HOIST_EACH_GROUP);
        // the tables are read before the call returns (the upload waits on the stream for the launch that read the last ones)
        if (int rc = hoist_upload_tables(p, L, giant_elements + t0, giant_keys + t0 * L, gt, {}, ws + d.inner.h.table, s)) return rc;
        bool skip_diag = false;
        for (size_t r0 = 0; r0 < gt;) {
            if (giant_elements[t0 + r0] == 1) { r0++; continue; }
            size_t r1 = r0 + 1;
            while (r1 < gt && giant_elements[t0 + r1] != 1) r1++;
            // a run of giant steps with a key: ONE polynomial per item through the tail of troyn_switch_key, then decomposed as a target
            const size_t run = (r1 - r0) * batch;
            KsLayout w = k;
            w.poly_prod = k.poly_prod + (t0 + r0) * batch * x_item;
            w.target_intt = k.target_intt + r0 * batch * v_item;
            w.temp_ntt = k.temp_ntt + r0 * batch * digit_item;
            u64* v = ws + d.v + r0 * batch * v_item;
            KsCall vc{p, L, is_ckks, ntt, v, v_item, TROYN_ASSIGN_OVERWRITE, v, nullptr, 0, ws, w, run, s, nullptr, v, v_item};
            vc.comps = 1;
            if (int rc = ks_tail(vc, ks_path(p, L, run, ntt, false))) return rc;
            if (int rc = hoist_decompose(vc, skip_diag)) return rc;
            r0 = r1;
        }
        HoistDoubleArgs a;
        std::memset(&a, 0, sizeof(a));
        a.mods = p->d_mods; a.K = K; a.L = L; a.log_n = p->log_n; a.batch = (unsigned)batch; a.groups = (unsigned)groups;
        a.terms = (unsigned)gt; a.accumulate = t0 ? 1 : 0;
        a.digits_ntt = ws + k.temp_ntt; a.v_ntt = ws + d.v; a.diag_from_v = skip_diag ? 1 : 0;
        a.x_ntt = ws + k.poly_prod + t0 * batch * x_item;
        a.keys = reinterpret_cast<const u64* const*>(ws + d.inner.h.table);
        a.elements = ws + d.inner.h.table + gt * L;
        a.poly_prod = ws + d.y;
        {
            TimerScope ts(TROYN_TIMER_KS_INNER_PRODUCT, s);
            const dim3 grid((unsigned)(rows * ch)), block(POLY_BLOCK);
            if (ib == 4) hipLaunchKernelGGL((hoist_double_kernel<4>), grid, block, 0, s, ch, a);
            else if (ib == 2) hipLaunchKernelGGL((hoist_double_kernel<2>), grid, block, 0, s, ch, a);
            else hipLaunchKernelGGL((hoist_double_kernel<1>), grid, block, 0, s, ch, a);
            LAUNCH_CHECK();
        }
    }
    // the tail of troyn_switch_key on `batch` items, both components overwritten: the ONE division of the transform
    const u64* c1 = ct + (size_t)L * n;
    KsLayout wy = k;
    wy.poly_prod = d.y;
    KsCall tc{p, L, is_ckks, ntt, c1, ct_words, TROYN_ASSIGN_OVERWRITE, out, nullptr, 0, ws, wy, batch, s, nullptr, c1, ct_words};
    return ks_tail(tc, ks_path(p, L, batch, ntt, false));
}

// ---------------------------------------------------------------------------------------
// modulus switching
// ---------------------------------------------------------------------------------------
extern "C" int troyn_divide_and_round_q_last(const troyn_plan* p, uint32_t L, const uint64_t* in, size_t pcount,
                                             uint64_t* out, size_t batch, troyn_stream_t stream) {
    select_device(p);
    if (!p || !in || !out) return fail(TROYN_E_INVALID, "[RNSTool::divide_and_round_q_last] null argument");
    if (L < 2 || L > p->K) return fail(TROYN_E_INVALID, "[Evaluator::mod_switch_scale_to_next_internal] Next context data is not set.");
    const size_t items = batch * pcount, rows = items * (L - 1);
    if (rows == 0) return TROYN_OK;
    const unsigned ch = chunks_pairs(p->n);
    if (int rc = check_rows(rows, ch)) return rc;
    hipLaunchKernelGGL(divide_round_q_last_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, (hipStream_t)stream,
                       ch, p->d_mods, L, p->n, (const u64*)in, p->d_inv_last + (size_t)L * p->K, (u64*)out);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" size_t troyn_divide_and_round_q_last_ntt_workspace_bytes(const troyn_plan* p, uint32_t L, size_t pcount, size_t batch) {
    if (!p || L < 1) return 0;
    return batch * pcount * (size_t)(2 * L - 1) * p->n * sizeof(u64);   // last_intt [items][N] + 2 x temp [items][L-1][N]
}

extern "C" int troyn_divide_and_round_q_last_ntt(const troyn_plan* p, uint32_t L, const uint64_t* in, size_t pcount,
                                                 uint64_t* out, void* workspace, size_t workspace_bytes,
                                                 size_t batch, troyn_stream_t stream) {
    select_device(p);
    if (!p || !in || !out || !workspace) return fail(TROYN_E_INVALID, "[RNSTool::divide_and_round_q_last_ntt] null argument");
    if (L < 2 || L > p->K) return fail(TROYN_E_INVALID, "[Evaluator::mod_switch_scale_to_next_internal] Next context data is not set.");
    if (workspace_bytes < troyn_divide_and_round_q_last_ntt_workspace_bytes(p, L, pcount, batch))
        return fail(TROYN_E_WORKSPACE, "[troyn_divide_and_round_q_last_ntt] workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const size_t items = batch * pcount, n = p->n;
    if (items == 0) return TROYN_OK;
    u64* last_intt = (u64*)workspace;
    u64* temp0 = last_intt + items * n;               // step1 output (coefficient form)
    u64* temp = temp0 + items * (size_t)(L - 1) * n;  // its NTT (out of place: lets the NTT use half-limb workgroups)
    int rc;
    // INTT of the last limb only (the reference's device branch transforms all L limbs, utils/rns_tool.cu:675)
    NttArgs li = contiguous_args(p, (const u64*)in + (size_t)(L - 1) * n, last_intt, 1, 1, L - 1, 1, TROYN_IDX_COMPONENTWISE, 0);
    li.in_bstride = (long long)L * n;
    // step1 -> NTT -> step2 in one launch (prologue / epilogue of the forward transform)
    NttArgs fw = contiguous_args(p, last_intt, (u64*)out, 1, L - 1, 0, L - 1, TROYN_IDX_COMPONENTWISE, 0);
    fw.in_bstride = (long long)n; fw.in_pstride = 0; fw.in_cstride = 0;
    fw.load_mode = NTT_LOAD_RESCALE; fw.aux_mod = L - 1;
    fw.store_mode = NTT_STORE_RESCALE;
    fw.ext0 = (const u64*)in; fw.ext0_bstride = (long long)L * n; fw.ext0_pstride = 0; fw.ext0_cstride = n;
    fw.inv_table = p->d_inv_last + (size_t)L * p->K;
    // a few ciphertexts at N = 16384: three launches instead of four (small_tail; the pass in between lives in `out`, as in the two-pass form)
    if (small_tail_wanted(p, items * (L - 1))) return small_tail(p, use_f64(p, 0, L), li, items, fw, (u64*)out, items, s);
    if ((rc = launch_ntt(p, li, items, true, s))) return rc;
    if (p->log_n >= 10) return launch_ntt(p, fw, items, false, s);
    const unsigned ch = chunks_pairs(p->n);
    const size_t rows = items * (L - 1);
    if ((rc = check_rows(rows, ch))) return rc;
    hipLaunchKernelGGL(rescale_step1_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s, ch, p->d_mods, L, p->n, last_intt, temp0);
    LAUNCH_CHECK();
    {
        NttArgs a = contiguous_args(p, temp0, temp, 1, L - 1, 0, L - 1, TROYN_IDX_COMPONENTWISE, 0);
        if ((rc = launch_ntt(p, a, items, false, s))) return rc;
    }
    hipLaunchKernelGGL(rescale_step2_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s, ch, p->d_mods, L, p->n,
                       (const u64*)in, temp, p->d_inv_last + (size_t)L * p->K, (u64*)out);
    LAUNCH_CHECK();
    return TROYN_OK;
}

// ---------------------------------------------------------------------------------------
// fused CKKS multiply -> relinearize -> rescale_to_next
// ---------------------------------------------------------------------------------------
struct MrrLayout { size_t digits, poly_prod, spec_intt, last_intt, keys_f64, keys_int, split, fast_total, prod3, relin2, sub, total; };

// the moduli the chain of level L touches (data limbs 0 .. L-1 and the special prime K-1) are all below 2^50 and the FP64 policy is not switched off
static bool mrr_all_f64(const troyn_plan* p, uint32_t L) { return use_f64(p, 0, L) && use_f64(p, p->K - 1, 1); }

static bool mrr_fast_path(const troyn_plan* p, uint32_t L) {
    // the chain's kernels exist for N = 8192 / 16384 / 32768 (d_fwd_r2); every modulus below 2^50: the FP64 kernels of rounds 2-4; chains with
    // moduli of 2^50 and more (round 5): every launch runs per modulus class, integer kernels for the wide limbs (ksmaci_kernel, the integer
    // forms of the fused transforms).  TROYN_MRR_MIXED=0 composes the three public calls for such chains as rounds 2-4 did (A/B runs, tests).
    if (!(p->d_fwd_r2 && L >= 2 && L + 1 <= p->K)) return false;
    if (mrr_all_f64(p, L)) return true;
    return p->d_fwd_r2i != nullptr && L + 1 <= 64 && !p->opt.mrr_mixed_off;
}

static MrrLayout mrr_layout(const troyn_plan* p, uint32_t L, size_t batch) {
    const size_t n = p->n;
    MrrLayout w;
    size_t off = 0;
    w.digits = off;    off += batch * L * n;
    w.poly_prod = off; off += batch * 2 * (size_t)(L + 1) * n;
    w.spec_intt = off; off += batch * 2 * n;
    w.last_intt = off; off += batch * 2 * n;
    w.keys_f64 = off;  off += (size_t)L * 2 * p->K * n + (size_t)L * 2 * n;     // prepared keys + the diagonal blocks in natural order
    // integer rows of a chain with wide moduli: (key, quotient) pairs [L][2][rows][N] + the diagonal blocks [rows][2][N]
    w.keys_int = off;  off += (L >= 1 && L + 1 <= p->K && !mrr_all_f64(p, L)) ? ((size_t)L * 2 * (L + 1) * n + (size_t)(L + 1) * 2 * n) * 2 : 0;
    w.split = off;     off += ks_split_words(p, batch, L, p->log_n);                        // slots of the digit-parallel inner product (small batches)
    w.fast_total = off;
    // composition of the three public calls (any other shape)
    off = 0;
    w.prod3 = off;  off += batch * 3 * (size_t)L * n;
    w.relin2 = off; off += batch * 2 * (size_t)L * n;
    w.sub = off;
    const size_t sub_bytes = std::max(troyn_relinearize_workspace_bytes(p, L, batch), troyn_divide_and_round_q_last_ntt_workspace_bytes(p, L, 2, batch));
    off += (sub_bytes + 7) / 8;
    w.total = std::max(off, w.fast_total);
    return w;
}

// internal streams of the chunked chain: one pair per (host thread, device), created on first use and kept for the life of the thread
constexpr int MRR_MAX_STREAMS = 4;
struct MrrStreams { hipStream_t s[MRR_MAX_STREAMS] = {}; hipEvent_t fork = nullptr, join[MRR_MAX_STREAMS] = {}; int device = -1; };
static MrrStreams* mrr_streams(int device) {
    static thread_local std::vector<MrrStreams> pool;
    for (auto& m : pool) if (m.device == device) return &m;
    MrrStreams m;
    m.device = device;
    bool ok = true;
    for (int q = 0; q < MRR_MAX_STREAMS && ok; q++) {
        ok = hipStreamCreateWithFlags(&m.s[q], hipStreamNonBlocking) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&m.join[q], hipEventDisableTiming) == hipSuccess;
    }
    ok = ok && hipEventCreateWithFlags(&m.fork, hipEventDisableTiming) == hipSuccess;
    if (!ok) {      // give back whatever was created before the failure
        for (int q = 0; q < MRR_MAX_STREAMS; q++) {
            if (m.join[q]) (void)hipEventDestroy(m.join[q]);
            if (m.s[q]) (void)hipStreamDestroy(m.s[q]);
        }
        if (m.fork) (void)hipEventDestroy(m.fork);
        return nullptr;
    }
    pool.push_back(m);      // kept for the life of the host thread (a handful of streams per thread and device; the runtime reclaims them at exit)
    return &pool.back();
}

// ksmac2's NLC instantiation (half tiles, N = 16384, all-FP64 fused chain): the words of a digit enter layer 0 as they are (u, v < max q_j), leave it
// as |x| <= max q_j + 0.875 p and run the three layers of round 0 without a re-centring in between.  Growth per layer: |x'| <= |x| + (0.5 + 1.5 |x| 2^-52) p
// (dev_math_f64.hpp); the chain qualifies when every value stays below 2^53 with a 2 % margin for EVERY row modulus p of the launch.
static bool ksmac_no_load_corr_ok(const troyn_plan* p, unsigned L) {
    if (p->log_n != 14 || p->opt.ntt_u64) return false;
    double qmax = 0.0;
    for (unsigned j = 0; j < L; j++) qmax = std::max(qmax, (double)p->moduli[j]);
    for (unsigned k = 0; k <= L; k++) {
        const double pm = (double)p->moduli[k == L ? p->K - 1 : k];
        double a = qmax + 0.875 * pm;
        for (int layer = 0; layer < 3; layer++) a += (0.5 + 1.5 * a * 0x1p-52) * pm;
        if (!(a < 0.98 * 0x1p53)) return false;
    }
    return true;
}

// ki: the integer rows' prepared keys (chains with wide moduli; nullptr otherwise); rows: ks_rows(p, L), the masks the keys were prepared for
struct MrrCall {
    const troyn_plan* p; uint32_t L; const u64* a; const u64* b; u64* out; u64* ws; const MrrLayout& w; size_t batch; hipStream_t s;
    bool all_f64, special_wide, last_wide;                               // classes of the chain, of the special prime, of the dropped limb
    unsigned t_flags() const { return (special_wide ? NTT_FLAG_TS_U64 : 0u) | (last_wide ? NTT_FLAG_TL_U64 : 0u); }
    long long ct_b() const { return 2ll * L * p->n; }                     // strides of a, b
    long long ct_p() const { return (long long)L * p->n; }
    u64* poly_prod() const { return ws + w.poly_prod; }
    // runs of data limbs [j0, j1) of one class within [0, count); runs of different classes in flight together (RunOverlap above)
    template <typename F> int for_runs(unsigned count, unsigned polys, F&& f) const {
        return for_class_runs(p, 0, count, class_by_policy, !all_f64 && batch * (size_t)polys * count >= OVERLAP_MIN_LIMB_POLYS, s, f);
    }
};

// the launches mrr_tail_kernel serves: N = 16384, an all-FP64 chain, a batch beyond the small-batch forms (mrr_chain's choice of the tail)
static bool mrr_whole_limb_class(const MrrCall& c) {
    const troyn_plan* p = c.p;
    return c.all_f64 && p->log_n == 14 && !p->opt.mrr_small_off && !small_tail_wanted(p, c.batch * 2 * (size_t)(c.L - 1));
}

// (1) digits = INTT(c2), c2 = a1 (.) b1 formed in the loader (kernel_dyadic_convolute's third output + transform_from_ntt, :817-821)
static int mrr_digits(const MrrCall& c) {
    const troyn_plan* p = c.p; const unsigned L = c.L, n = p->n;
    if (mrr_whole_limb_class(c) && !p->opt.mulpair_half_off && p->d_inv_r2) {
        // the class of the merged whole-limb tail: half-limb tiles, two workgroups per CU (troyn_mulpair_half.hip; TROYN_MULPAIR_HALF=0: the kernel below)
        MulpairHalfArgs x;
        x.a1 = c.a + c.ct_p(); x.b1 = c.b + c.ct_p(); x.in_bstride = c.ct_b();
        x.out = c.ws + c.w.digits; x.out_bstride = (long long)L * n;
        x.mods = p->d_mods; x.tw = p->d_inv_f64; x.tw_r1 = p->d_inv_r1; x.tw_r2 = p->d_inv_r2;
        x.L = L; x.store_f64 = 1u;          // all-FP64: the digits go to ksmac2 as doubles
        if (!launch_mulpair_half(p->log_n, c.batch, x, c.s)) return fail(TROYN_E_INVALID, "[troyn_ckks_multiply_relinearize_rescale] batch too large for one launch");
        LAUNCH_CHECK();
        return TROYN_OK;
    }
    return c.for_runs(L, 1, [&](unsigned j0, unsigned j1, hipStream_t rs) {
        NttArgs x = contiguous_args(p, c.a + (size_t)j0 * n, c.ws + c.w.digits + (size_t)j0 * n, 1, j1 - j0, j0, j1 - j0, TROYN_IDX_COMPONENTWISE, 0);
        x.in_bstride = c.ct_b(); x.in_pstride = c.ct_p();                  // (the loader reads mul_a / mul_b; `in` only anchors the shapes)
        x.out_bstride = (long long)L * n; x.out_pstride = (long long)L * n;
        x.mul_a = c.a; x.mul_b = c.b; x.mul_bstride = c.ct_b(); x.mul_pstride = c.ct_p(); x.mul_limb0 = j0;
        x.fused_mode = NTT_FUSED_MULPAIR;
        if (c.all_f64) x.flags = NTT_FLAG_STORE_F64;          // the digits go to ksmac2 as doubles (one conversion here instead of L + 1 there)
        return launch_ntt(p, x, c.batch, true, rs);
    });
}

// (2) key-switch inner product; the digit of row k under its own modulus is a1 (.) b1 again
static int mrr_inner_product(const MrrCall& c, const KsRows& rows, const double* kf, const ulonglong2* ki, const KeyPtrs* raw) {
    const troyn_plan* p = c.p; const unsigned L = c.L, K = p->K, n = p->n;
    TimerScope ts(TROYN_TIMER_KS_INNER_PRODUCT, c.s);
    if (rows.small) {
        KsMacArgs m = ksmac2_args(p, L, c.batch, c.ws + c.w.digits, (long long)L * n, c.poly_prod(), kf);
        m.diag = c.a + c.ct_p(); m.diag_b = c.b + c.ct_p(); m.diag_bstride = c.ct_b(); m.diag_cstride = n;
        m.ten_a = c.a; m.ten_b = c.b; m.ten_bstride = c.ct_b(); m.ten_pstride = c.ct_p();      // data rows leave as Q = P qk^-1 + c (keys prepared times qk^-1)
        m.diag_keys = kf + (size_t)L * 2 * K * n;
        if (rows.wide) m.row_mask = rows.small;
        m.no_load_corr = (c.all_f64 && ksmac_no_load_corr_ok(p, L)) ? 1u : 0u;
        if (raw) {
            m.grouped = 0;
            m.part = reinterpret_cast<double*>(c.ws + c.w.split); m.part_jstride = (long long)c.batch * m.out_bstride;
            m.split_skip_diag = 1;
            m.raw = *raw; m.raw_pstride = (long long)K * n; m.split_scale = p->d_inv_last + (size_t)K * K;
            launch_ksmac2_split(p->log_n, c.batch, m, c.s, true, 1);
        } else launch_ksmac2(p->log_n, c.batch, (unsigned)__builtin_popcountll(rows.small), m, c.s, c.all_f64, rows.wide_digits);
        LAUNCH_CHECK();
    }
    if (rows.wide) {
        KsMacIArgs m = ksmaci_args(p, L, c.batch, c.ws + c.w.digits, (long long)L * n, c.poly_prod(), ki, rows.wide);
        m.ten_a = c.a; m.ten_b = c.b; m.ten_bstride = c.ct_b(); m.ten_pstride = c.ct_p();
        launch_ksmaci(p->log_n, c.batch, m, c.s, 2);
        LAUNCH_CHECK();
    }
    return TROYN_OK;
}

// arguments of steps (4) and (5) (also read by the merged forms of the tail)
static NttArgs mrr_last_args(const MrrCall& c) {
    const troyn_plan* p = c.p; const unsigned L = c.L, K = p->K, n = p->n;
    NttArgs x = contiguous_args(p, c.poly_prod() + (size_t)(L - 1) * n, c.ws + c.w.last_intt, 2, 1, L - 1, 1, TROYN_IDX_COMPONENTWISE, 0);
    x.in_pstride = (long long)(L + 1) * n; x.in_bstride = 2ll * (L + 1) * n;
    x.in2 = c.ws + c.w.spec_intt; x.in2_bstride = 2ll * n; x.in2_pstride = n;
    x.aux_mod = K - 1; x.inv_table = p->d_inv_last + (size_t)K * K + (L - 1);
    x.fused_mode = (!c.last_wide && c.special_wide) ? NTT_FUSED_LAST_LIMB_W : NTT_FUSED_LAST_LIMB;
    x.flags = c.t_flags();
    return x;
}
static NttArgs mrr_tail_args(const MrrCall& c, unsigned j0, unsigned j1) {
    const troyn_plan* p = c.p; const unsigned L = c.L, K = p->K, n = p->n;
    NttArgs x = contiguous_args(p, c.ws + c.w.spec_intt, c.out + (size_t)j0 * n, 2, j1 - j0, j0, j1 - j0, TROYN_IDX_COMPONENTWISE, 0);
    x.in_bstride = 2ll * n; x.in_pstride = n; x.in_cstride = 0;
    x.out_bstride = 2ll * (L - 1) * n; x.out_pstride = (long long)(L - 1) * n;
    x.in2 = c.ws + c.w.last_intt; x.in2_bstride = 2ll * n; x.in2_pstride = n;
    x.aux_mod = K - 1; x.inv_table = p->d_inv_last + (size_t)K * K + j0;
    x.aux2_mod = L - 1; x.inv_table2 = p->d_inv_last + (size_t)L * K + j0;
    x.ext0 = c.poly_prod() + (size_t)j0 * n; x.ext0_bstride = 2ll * (L + 1) * n; x.ext0_pstride = (long long)(L + 1) * n; x.ext0_cstride = n;
    x.fused_mode = (class_by_policy(p, j0) && c.t_flags()) ? NTT_FUSED_TAIL_RESCALE_W : NTT_FUSED_TAIL_RESCALE;     // (launch_ntt co-locates the limbs that share the two input rows on one XCD)
    x.flags = c.t_flags();
    return x;
}

// The merged forms of the tail (all-FP64 chains), T_s and T_l in registers: steps (3)-(5) on the special rows, the dropped limb and all L - 1 output limbs.
//   quartet (troyn_mrr_small.hip): single objects at N = 16384 (every launch of the tail in its two-pass form): the three strided passes between
//     the first inverse pass of {limb L-1, special rows} and the last forward pass of the output limbs run as ONE launch: 3 launches instead of 6.
//     N = 32768 (two-pass transforms at every size): this form at EVERY batch -- T_s and T_l never reach memory, three strided passes become one
//     (one thread per octet loops over the output limbs when the launch is not small): fused chain 6 x 50-bit, 256 items 117.5 k -> 126 k ops/s
//   whole-limb (troyn_mrr_tail.hip): N = 16384, batches that fill the chip: ONE launch, one workgroup per (item, polynomial) -- the spec_intt /
//     last_intt rows are not touched.
// TROYN_MRR_SMALL=0 keeps the six / three launches.
static int mrr_tail_merged(const MrrCall& c, bool quartet) {
    const troyn_plan* p = c.p; const unsigned L = c.L, K = p->K, n = p->n;
    const LaunchCtx lc = launch_ctx(p, c.s);
    if (quartet) {
        // first inverse pass of rows L-1 and L (special) of both polynomials, in place in poly_prod (nothing else reads those rows)
        u64* rows = c.poly_prod() + (size_t)(L - 1) * n;
        NttArgs pa = contiguous_args(p, rows, rows, 2, 2, L - 1, K - (L - 1), TROYN_IDX_KS_SKIP_FINALS, 1);
        pa.in_pstride = pa.out_pstride = (long long)(L + 1) * n; pa.in_bstride = pa.out_bstride = 2ll * (L + 1) * n;
        prep_direct(p, pa, true, true);
        launch_small_pass(p->log_n, true, 0, pa, c.batch * 4, lc);
        LAUNCH_CHECK();
    }
    NttArgs sp = special_rows_args(p, c.poly_prod(), nullptr, L);
    prep_direct(p, sp, true, true);
    NttArgs la = mrr_last_args(c);
    prep_direct(p, la, true, true);
    NttArgs ta = mrr_tail_args(c, 0, L - 1);
    prep_direct(p, ta, true, false);
    if (!quartet) {
        launch_mrr_tail(p->log_n, c.batch, sp, la, ta, c.s);
        LAUNCH_CHECK();
        return TROYN_OK;
    }
    launch_mrr_quartet(p->log_n, c.batch, sp, la, ta, c.s, !p->opt.mrr_small_serial && is_small_launch(c.batch * 2 * (size_t)(L - 1)));
    LAUNCH_CHECK();
    // last forward pass of the output limbs, in place in `out`, with step (5)'s epilogue
    as_input_of(ta, ta);
    ta.reduce_input = 0;
    launch_small_pass(p->log_n, true, 1, ta, c.batch * 2 * (L - 1), lc);
    LAUNCH_CHECK();
    return TROYN_OK;
}

// launches (1)-(5) of the fused chain for `batch` items whose intermediates live in `ws` (layout w); kf: the prepared keys
// raw != nullptr: digit-parallel inner product on the caller's own keys (small launches; the workspace has its slots and kf was not prepared)
// Chains with moduli of 2^50 and more: every launch is issued once per run of limbs of one arithmetic class (limbs are independent), the rows
// that cross classes are canonical u64 words (digits; T rows written by an integer kernel) and each consumer reduces what it reads.
static int mrr_chain(const troyn_plan* p, uint32_t L, const KsRows& rows, const u64* a, const u64* b, const double* kf, const ulonglong2* ki, u64* out, u64* ws,
                     const MrrLayout& w, size_t batch, hipStream_t s, const KeyPtrs* raw = nullptr) {
    const MrrCall c{p, L, a, b, out, ws, w, batch, s, mrr_all_f64(p, L), !class_by_policy(p, p->K - 1), !class_by_policy(p, L - 1)};
    int rc;
    if ((rc = mrr_digits(c))) return rc;
    if ((rc = mrr_inner_product(c, rows, kf, ki, raw))) return rc;
    if (c.all_f64 && (small_tail_wanted(p, batch * 2 * (size_t)(L - 1)) || (p->log_n == 15 && !p->opt.mrr_small_off))) return mrr_tail_merged(c, true);
    if (mrr_whole_limb_class(c)) return mrr_tail_merged(c, false);
    // (3) s = INTT of the special-prime rows (:991-996, only the two rows the NTT-form tail needs)
    {
        NttArgs x = special_rows_args(p, c.poly_prod(), ws + w.spec_intt, L);
        x.flags = NTT_FLAG_STORE_ROUND_HALF;     // stored as (s + qk/2) mod qk, the limb-independent part of the key switch's rounding fix
        if ((rc = launch_ntt(p, x, batch, true, s))) return rc;
    }
    // (4) l = INTT(relin_{L-1}) = INTT(Q_{L-1}) - r(s) qk^-1 with Q = P qk^-1 + c as ksmac2 left it   (divide_and_round_q_last_ntt's INTT of the last limb, :675)
    if ((rc = launch_ntt(p, mrr_last_args(c), batch, true, s))) return rc;
    // (5) out_j = (Q_j - NTT_j(r_j(s) qk^-1 + f_j(l))) ql^-1, Q_j = P_j qk^-1 + c_j, for the L-1 remaining limbs: ski_util6/7 (:570-658), the
    //     trailing add of relinearize (:143) and both steps of divide_and_round_q_last_ntt (utils/rns_tool.cu:523-627) around ONE transform
    return c.for_runs(L - 1, 2, [&](unsigned j0, unsigned j1, hipStream_t rs) { return launch_ntt(p, mrr_tail_args(c, j0, j1), batch, false, rs); });
}

extern "C" size_t troyn_ckks_multiply_relinearize_rescale_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t batch) {
    if (!plan || L < 2 || L > plan->K) return 0;
    return mrr_layout(plan, L, batch).total * sizeof(u64);
}

extern "C" int troyn_ckks_multiply_relinearize_rescale(const troyn_plan* p, uint32_t L, const uint64_t* a_, const uint64_t* b_,
                                                       const uint64_t* const* keys, uint64_t* out_, void* workspace, size_t workspace_bytes,
                                                       size_t batch, troyn_stream_t stream) {
    select_device(p);
    const char* P = "[troyn_ckks_multiply_relinearize_rescale]";
    if (!p || !a_ || !b_ || !keys || !out_ || !workspace) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    const unsigned K = p->K, n = p->n;
    if (K < 2) return fail(TROYN_E_INVALID, "[Evaluator::switch_key_inplace_internal] Keyswitching is not supported.");
    if (L < 2 || L > K - 1) return fail(TROYN_E_INVALID, "[Evaluator::mod_switch_scale_to_next_internal] Next context data is not set.");
    const MrrLayout w = mrr_layout(p, L, batch);
    if (workspace_bytes < w.total * sizeof(u64)) return fail(TROYN_E_WORKSPACE, std::string(P) + " workspace too small");
    if (batch == 0) return TROYN_OK;
    hipStream_t s = (hipStream_t)stream;
    const u64* a = (const u64*)a_; const u64* b = (const u64*)b_;
    u64* out = (u64*)out_;
    u64* ws = (u64*)workspace;
    int rc;
    const bool unfused = p->opt.mrr_calls;    // TROYN_MRR=calls: composes the three public calls (A/B testing)
    // (a few ciphertexts of a chain with moduli >= 2^50: the three calls, whose key switch then takes the two-launch inner product -- ks_small_mixed)
    if (!mrr_fast_path(p, L) || unfused || ks_small_mixed(p, L, batch) || batch * (size_t)(L + 1) * 4 > 0x7fffffffull) {
        // Evaluator::multiply (evaluator.cu:118-145) -> relinearize (evaluator_keyswitching.cu:119-144) -> rescale_to_next
        if ((rc = launch_convolute(p->d_mods, n, 0, L, a, 2, b, 2, ws + w.prod3, batch, s))) return rc;
        const size_t sub_bytes = (w.total - w.sub) * sizeof(u64);
        if ((rc = troyn_relinearize(p, L, 1, 1, (const uint64_t*)(ws + w.prod3), keys, (uint64_t*)(ws + w.relin2), ws + w.sub, sub_bytes, batch, stream))) return rc;
        return troyn_divide_and_round_q_last_ntt(p, L, (const uint64_t*)(ws + w.relin2), 2, out_, ws + w.sub, sub_bytes, batch, stream);
    }
    KeyPtrs kp;
    std::memset(&kp, 0, sizeof(kp));
    for (unsigned j = 0; j < L; j++) {
        if (!keys[j]) return fail(TROYN_E_INVALID, "[Evaluator::switch_key_inplace_internal] null key pointer");
        kp.p[j] = (const u64*)keys[j];
    }
    const int chunk_env = p->opt.mrr_chunk;
    size_t chunk = batch;
    if (chunk_env > 0 && batch >= 2 * (size_t)chunk_env && (chunk_env % 8) == 0) chunk = (size_t)chunk_env;
    const bool all_f64 = mrr_all_f64(p, L);
    // small launches: the digit-parallel inner product reads the caller's keys as they are (chains of moduli below 2^50)
    const bool split = chunk == batch && all_f64 && ksmac_split_wanted(p, batch, L, p->log_n);
    // otherwise: keys prepared once per call (converted to exact doubles in the accumulators' layout), shared by every chunk
    double* kf = reinterpret_cast<double*>(ws + w.keys_f64);
    ulonglong2* ki = reinterpret_cast<ulonglong2*>(ws + w.keys_int);
    const KsRows rows = ks_rows(p, L);                   // once per call: preparation and every chunk's launches read the same masks
    // the rows of the data moduli carry the factor qk^-1: the inner product leaves ksmac2 as P qk^-1 (+ the tensor term, KsMacArgs::ten_a)
    if (!split && rows.small && (rc = prepare_keys_f64(p, kp, L, kf, L, true, s))) return rc;
    // the integer rows' (key qk^-1, Shoup quotient) pairs in the accumulators' layout + their diagonal blocks in natural order
    if (rows.wide && (rc = prepare_keys_int(p, kp, L, rows.wide, ki, L, true, s))) return rc;
    // Chunked execution of the 5-launch chain on internal streams (round 3, an option: TROYN_MRR_CHUNK=<items, multiple of 8>,
    // TROYN_MRR_STREAMS=<1..4>, default 2): the batch is cut into chunks that alternate on internal streams, forked from and joined to
    // the caller's stream by events; chunks are independent (the batch is), results are unchanged.  The kernels of one chunk bound
    // differently (the inner product by FP64 issue, the transforms by memory), so two chunks in flight fill each other's idle resource:
    // +3 % when it was introduced.  Since then the inner product and the tail place the workgroups that share rows on one XCD (band
    // order; polynomials of a limb back to back) and a second chunk's kernels evict exactly those rows from the L2: one chunk on the
    // caller's stream is faster at every batch size measured (1024 items: 263.6 - 265.2 k vs 260.4 - 260.8 k ops/s with two halves,
    // 263.2 - 264.1 k with three thirds; 2048: 264.1 - 264.6 k vs 260.1 - 262.7 k; 512: 262.3 - 262.9 k vs 257.4 - 258.1 k) and is the default.
    const int ns = std::min(std::max(p->opt.mrr_streams, 1), MRR_MAX_STREAMS);
    if (chunk == batch) return mrr_chain(p, L, rows, a, b, kf, ki, out, ws, w, batch, s, split ? &kp : nullptr);
    MrrStreams* ms = mrr_streams(p->device);
    if (!ms) return fail(TROYN_E_INVALID, std::string(P) + " cannot create the internal streams");
    const MrrLayout wc = mrr_layout(p, L, chunk);        // two chunk-sized workspaces side by side in the caller's workspace
    const size_t slot_words = wc.keys_f64;               // a chunk's intermediates end where its (unused) key area would start
    if ((size_t)ns * slot_words > w.keys_f64) {
        if (split) return fail(TROYN_E_INVALID, std::string(P) + " internal: chunk layout");      // unreachable: split implies one chunk
        return mrr_chain(p, L, rows, a, b, kf, ki, out, ws, w, batch, s);
    }
    HIP_TRY(hipEventRecord(ms->fork, s));
    for (int q = 0; q < ns; q++) HIP_TRY(hipStreamWaitEvent(ms->s[q], ms->fork, 0));
    size_t done = 0, idx = 0;
    rc = TROYN_OK;
    while (done < batch) {
        const size_t c = std::min(chunk, batch - done);
        const int q = (int)(idx % (size_t)ns);
        if ((rc = mrr_chain(p, L, rows, a + done * 2 * (size_t)L * n, b + done * 2 * (size_t)L * n, kf, ki, out + done * 2 * (size_t)(L - 1) * n,
                            ws + (size_t)q * slot_words, wc, c, ms->s[q]))) break;
        done += c; idx++;
    }
    // join ALSO on an error: the chunks already queued keep writing the caller's workspace / output, so the caller's stream must not
    // run ahead of them (the caller is free to release both as soon as this returns)
    bool joined = true;
    for (int q = 0; q < ns; q++)
        joined = hipEventRecord(ms->join[q], ms->s[q]) == hipSuccess && hipStreamWaitEvent(s, ms->join[q], 0) == hipSuccess && joined;
    if (!joined) { for (int q = 0; q < ns; q++) (void)hipStreamSynchronize(ms->s[q]); }
    return rc;
}

// Dot product of ciphertexts with lazy relinearization (an addition): SUM_t a[t] (x) b[t] into the workspace, then the drivers of troyn_relinearize
// and troyn_divide_and_round_q_last_ntt on that buffer -- one key switch and one rescale for the whole sum.
//   workspace: prod3 [batch][3][L][N] | relin2 [batch][2][L][N] | the larger of the two drivers' own workspaces
struct MarrLayout { size_t prod3, relin2, sub, sub_bytes, total_bytes; };
static MarrLayout marr_layout(const troyn_plan* p, uint32_t L, size_t batch) {
    MarrLayout w;
    const size_t pc = (size_t)L * p->n;
    w.prod3 = 0;
    w.relin2 = batch * 3 * pc;
    w.sub = w.relin2 + batch * 2 * pc;
    w.sub_bytes = std::max(troyn_relinearize_workspace_bytes(p, L, batch), troyn_divide_and_round_q_last_ntt_workspace_bytes(p, L, 2, batch));
    w.total_bytes = w.sub * sizeof(u64) + w.sub_bytes;
    return w;
}

extern "C" size_t troyn_ckks_multiply_accumulate_relinearize_rescale_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t terms, size_t batch) {
    if (!plan || terms == 0 || plan->K < 2 || L < 2 || L > plan->K - 1) return 0;     // (the levels the entry itself refuses)
    return marr_layout(plan, L, batch).total_bytes;     // (the sum is formed in place: the size does not depend on `terms`)
}

extern "C" int troyn_ckks_multiply_accumulate_relinearize_rescale(const troyn_plan* p, uint32_t L, const uint64_t* const* a, const uint64_t* const* b,
                                                                  size_t terms, const uint64_t* const* keys, uint64_t* out, void* workspace,
                                                                  size_t workspace_bytes, size_t batch, troyn_stream_t stream) {
    select_device(p);
    const char* P = "[troyn_ckks_multiply_accumulate_relinearize_rescale]";
    if (!p || !a || !b || !keys) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (terms == 0) return fail(TROYN_E_INVALID, std::string(P) + " no terms");
    if (p->K < 2) return fail(TROYN_E_INVALID, "[Evaluator::switch_key_inplace_internal] Keyswitching is not supported.");
    if (L < 2 || L > p->K - 1) return fail(TROYN_E_INVALID, "[Evaluator::mod_switch_scale_to_next_internal] Next context data is not set.");
    const MarrLayout w = marr_layout(p, L, batch);
    if ((uintptr_t)workspace & 15) return fail(TROYN_E_INVALID, std::string(P) + " misaligned workspace");
    u64* ws = (u64*)workspace;
    // the operand tables first, as troyn_dyadic_convolute_accumulate does.  The sum is written to the workspace, so that is the buffer no operand
    // may overlap (`out` is written after the last read of the operands)
    if (int rc = check_convolute_accumulate(P, p, 0, L, a, b, terms, (const uint64_t*)ws, w.total_bytes / sizeof(u64), batch)) return rc;
    if (batch == 0) return TROYN_OK;      // as troyn_dyadic_convolute_accumulate: nothing to launch, `out` and the workspace are not looked at
    if (workspace_bytes < w.total_bytes) return fail(TROYN_E_WORKSPACE, std::string(P) + " workspace too small");
    if (!out) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    int rc;
    // SUM_t Evaluator::multiply (evaluator.cu:118-145) -> relinearize (evaluator_keyswitching.cu:119-144) -> rescale_to_next (utils/rns_tool.cu:499-694)
    if ((rc = launch_convolute_accumulate(p->d_mods, p->n, 0, L, a, b, terms, ws + w.prod3, 0, batch, (hipStream_t)stream))) return rc;
    if ((rc = troyn_relinearize(p, L, 1, 1, (const uint64_t*)(ws + w.prod3), keys, (uint64_t*)(ws + w.relin2), ws + w.sub, w.sub_bytes, batch, stream))) return rc;
    return troyn_divide_and_round_q_last_ntt(p, L, (const uint64_t*)(ws + w.relin2), 2, out, ws + w.sub, w.sub_bytes, batch, stream);
}

// Tensor product plus affine part, then the same two drivers (an addition: the Chebyshev recurrence and the double angle as ONE step).
//   workspace: the layout of the entry above (P is formed in prod3), then the scalar table [batch][L][4] = (alpha, w, k, 0)
static inline size_t maff_table_offset(const MarrLayout& w) { return (w.total_bytes + 15) & ~(size_t)15; }

extern "C" size_t troyn_ckks_multiply_affine_relinearize_rescale_workspace_bytes(const troyn_plan* plan, uint32_t L, size_t batch) {
    if (!plan || plan->K < 2 || L < 2 || L > plan->K - 1) return 0;     // (the levels the entry itself refuses)
    return maff_table_offset(marr_layout(plan, L, batch)) + batch * (size_t)L * 4 * sizeof(u64);
}

extern "C" int troyn_ckks_multiply_affine_relinearize_rescale(const troyn_plan* p, uint32_t L, const uint64_t* const* a, const uint64_t* const* b,
                                                              const uint64_t* const* c, const uint32_t* c_nmod, const uint64_t* alpha,
                                                              const uint64_t* weight, const uint64_t* constant, const uint64_t* const* keys,
                                                              uint64_t* out, void* workspace, size_t workspace_bytes, size_t batch,
                                                              troyn_stream_t stream) {
    select_device(p);
    const std::string P = "[troyn_ckks_multiply_affine_relinearize_rescale]";
    if (!p) return fail(TROYN_E_INVALID, P + " null argument");
    if (p->K < 2) return fail(TROYN_E_INVALID, "[Evaluator::switch_key_inplace_internal] Keyswitching is not supported.");
    if (L < 2 || L > p->K - 1) return fail(TROYN_E_INVALID, "[Evaluator::mod_switch_scale_to_next_internal] Next context data is not set.");
    if (batch == 0) return TROYN_OK;      // nothing to launch: no table, buffer or pointer entry is looked at
    if (!a || !b || !c || !c_nmod || !alpha || !weight || !keys || !out || !workspace) return fail(TROYN_E_INVALID, P + " null argument");
    if (((uintptr_t)out & 15) || ((uintptr_t)workspace & 15)) return fail(TROYN_E_INVALID, P + " misaligned destination or workspace");
    const unsigned n = p->n;
    const size_t pc = (size_t)L * n;
    const MarrLayout w = marr_layout(p, L, batch);
    const size_t tab_off = maff_table_offset(w), total = tab_off + batch * (size_t)L * 4 * sizeof(u64);
    // neither `out` nor the workspace (where P is formed while the operands are still being read) may overlap an operand
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + batch * 2 * (pc - n) * sizeof(u64);
    const uintptr_t w0 = (uintptr_t)workspace, w1 = w0 + total;
    if (o0 < w1 && w0 < o1) return fail(TROYN_E_INVALID, P + " out overlaps the workspace");
    for (size_t i = 0; i < batch; i++) {
        if (!a[i] || !b[i]) return fail(TROYN_E_INVALID, P + " null pointer in the operand tables");
        if (c[i] && c_nmod[i] < L) return fail(TROYN_E_INVALID, P + " an addend has fewer limbs than L");
        const uintptr_t q[3] = {(uintptr_t)a[i], (uintptr_t)b[i], (uintptr_t)c[i]};
        const size_t bytes[3] = {2 * pc * sizeof(u64), 2 * pc * sizeof(u64), c[i] ? 2 * (size_t)c_nmod[i] * n * sizeof(u64) : 0};
        for (int j = 0; j < 3; j++) {
            if (!q[j]) continue;
            if (q[j] & 15) return fail(TROYN_E_INVALID, P + " misaligned pointer in the tables");
            if (q[j] < o1 && o0 < q[j] + bytes[j]) return fail(TROYN_E_INVALID, P + " out overlaps an input");
            if (q[j] < w1 && w0 < q[j] + bytes[j]) return fail(TROYN_E_INVALID, P + " the workspace overlaps an input");
        }
        for (size_t l = 0; l < L; l++) {
            const u64 q_l = p->moduli[l];
            if (alpha[i * L + l] >= q_l || (c[i] && weight[i * L + l] >= q_l) || (constant && constant[i * L + l] >= q_l))
                return fail(TROYN_E_INVALID, P + " a scalar is not a canonical residue");
        }
    }
    if (workspace_bytes < total) return fail(TROYN_E_WORKSPACE, P + " workspace too small");
    const unsigned ch = chunks_pairs(n);
    if (int rc = check_rows(std::min<size_t>(batch, MAFF_MAX_ITEMS) * L, ch)) return rc;
    // the host tables are read here: one upload of (alpha, w, k, 0) per (item, limb)
    std::vector<u64> tab(batch * (size_t)L * 4, 0);
    for (size_t i = 0; i < batch * (size_t)L; i++) {
        tab[4 * i] = alpha[i];
        tab[4 * i + 1] = c[i / L] ? weight[i] : 0;
        tab[4 * i + 2] = constant ? constant[i] : 0;
    }
    hipStream_t s = (hipStream_t)stream;
    u64* ws = (u64*)workspace;
    const u64* d_tab = reinterpret_cast<const u64*>((const char*)workspace + tab_off);
    int rc;
    if ((rc = upload_host_table(s, (void*)d_tab, tab.data(), tab.size() * sizeof(u64)))) return rc;
    for (size_t i0 = 0; i0 < batch; i0 += MAFF_MAX_ITEMS) {
        const unsigned cnt = (unsigned)std::min<size_t>(batch - i0, MAFF_MAX_ITEMS);
        MulAffinePtrs g;
        for (unsigned i = 0; i < MAFF_MAX_ITEMS; i++) {
            const size_t j = i0 + (i < cnt ? i : 0);
            g.a[i] = reinterpret_cast<const u64*>(a[j]);
            g.b[i] = reinterpret_cast<const u64*>(b[j]);
            g.c[i] = reinterpret_cast<const u64*>(c[j]);
            g.c_nmod[i] = c[j] ? c_nmod[j] : 0;
        }
        hipLaunchKernelGGL(multiply_affine_kernel, dim3((unsigned)((size_t)cnt * L * ch)), dim3(POLY_BLOCK), 0, s, ch, p->d_mods, (unsigned)L, n, g,
                           d_tab + i0 * (size_t)L * 4, ws + w.prod3 + i0 * 3 * pc);
        LAUNCH_CHECK();
    }
    // Evaluator::relinearize (evaluator_keyswitching.cu:119-144) -> rescale_to_next (utils/rns_tool.cu:499-694), the drivers of the entry above
    if ((rc = troyn_relinearize(p, L, 1, 1, (const uint64_t*)(ws + w.prod3), keys, (uint64_t*)(ws + w.relin2), ws + w.sub, w.sub_bytes, batch, stream))) return rc;
    return troyn_divide_and_round_q_last_ntt(p, L, (const uint64_t*)(ws + w.relin2), 2, out, ws + w.sub, w.sub_bytes, batch, stream);
}

// Real and imaginary parts of CKKS slots (include/troyn.h): the rows of `batch` two-polynomial items on the plan's first L moduli
static int complex_rows(const troyn_plan* p, const std::string& P, uint32_t L, std::initializer_list<const void*> ptrs, size_t batch, size_t& rows, unsigned& ch) {
    if (!p) return fail(TROYN_E_INVALID, P + " null argument");
    if (L == 0 || L > p->K) return fail(TROYN_E_INVALID, P + " L outside [1, the plan's moduli]");
    rows = batch * 2 * (size_t)L;
    if (batch == 0) return TROYN_OK;      // nothing to launch: no pointer is looked at
    for (const void* q : ptrs) {
        if (!q) return fail(TROYN_E_INVALID, P + " null argument");
        if ((uintptr_t)q & 15) return fail(TROYN_E_INVALID, P + " misaligned pointer");
    }
    ch = chunks_pairs(p->n);
    return check_rows(rows, ch);
}

extern "C" int troyn_ckks_complex_split(const troyn_plan* p, uint32_t L, const uint64_t* a, const uint64_t* b, uint64_t* s, uint64_t* d, size_t batch,
                                        troyn_stream_t stream) {
    select_device(p);
    size_t rows = 0; unsigned ch = 1;
    if (int rc = complex_rows(p, "[troyn_ckks_complex_split]", L, {a, b, s, d}, batch, rows, ch)) return rc;
    if (rows == 0) return TROYN_OK;
    if (s == d) return fail(TROYN_E_INVALID, "[troyn_ckks_complex_split] s and d are the same buffer");
    hipLaunchKernelGGL(ckks_complex_split_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, (hipStream_t)stream, ch, p->d_mods, p->d_fwd, (unsigned)L, p->n,
                       (const u64*)a, (const u64*)b, (u64*)s, (u64*)d);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_ckks_complex_join(const troyn_plan* p, uint32_t L, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t batch, troyn_stream_t stream) {
    select_device(p);
    size_t rows = 0; unsigned ch = 1;
    if (int rc = complex_rows(p, "[troyn_ckks_complex_join]", L, {a, b, out}, batch, rows, ch)) return rc;
    if (rows == 0) return TROYN_OK;
    hipLaunchKernelGGL(ckks_complex_join_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, (hipStream_t)stream, ch, p->d_mods, p->d_fwd, (unsigned)L, p->n,
                       (const u64*)a, (const u64*)b, (u64*)out);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_mod_switch_drop(const troyn_plan* p, uint32_t L_in, uint32_t L_out, const uint64_t* in, size_t pcount,
                                     uint64_t* out, size_t batch, troyn_stream_t stream) {
    select_device(p);
    if (!p || !in || !out) return fail(TROYN_E_INVALID, "[Evaluator::mod_switch_drop_to_internal] null argument");
    if (L_out < 1 || L_out > L_in || L_in > p->K) return fail(TROYN_E_INVALID, "[Evaluator::mod_switch_drop_to_next_internal] Next context data is not set.");
    const size_t items = batch * pcount, rows = items * L_out;
    if (rows == 0) return TROYN_OK;
    const unsigned ch = chunks_pairs(p->n);
    if (int rc = check_rows(rows, ch)) return rc;
    hipLaunchKernelGGL(copy_limbs_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, (hipStream_t)stream,
                       ch, p->n, (const u64*)in, (size_t)L_in * p->n, 0u, (u64*)out, (size_t)L_out * p->n, L_out);
    LAUNCH_CHECK();
    return TROYN_OK;
}

// ---------------------------------------------------------------------------------------
// BGV: constants of one level's RNSTool that only BGV reads (utils/rns_tool.cu:205-232)
// ---------------------------------------------------------------------------------------
struct troyn_bgv {
    const troyn_plan* plan = nullptr;
    unsigned L = 0;
    u64 t = 0, inv_q_last_mod_t = 1, q_mod_t = 0;
    DevModulus t_mod;
    u64* d_consts = nullptr;            // [L] Shoup pairs (q/q_i)^-1 mod q_i, then [L] (q/q_i) mod t
    bool can_divide = false;            // q_last invertible mod t
};

extern "C" int troyn_bgv_destroy(troyn_bgv* b) {
    if (!b) return TROYN_OK;
    if (b->d_consts) (void)hipFree(b->d_consts);
    delete b;
    return TROYN_OK;
}

extern "C" int troyn_bgv_create(troyn_bgv** out, const troyn_plan* plan, uint32_t L, uint64_t t) {
    if (!out || !plan) return fail(TROYN_E_INVALID, "[troyn_bgv_create] null argument");
    *out = nullptr;
    if (L < 1 || L > plan->K) return fail(TROYN_E_INVALID, "[RNSTool::RNSTool] RNSBase length is invalid.");
    if (t < 2 || (t >> 61) != 0) return fail(TROYN_E_MODULUS, "[troyn_bgv_create] BGV needs a plain modulus in [2, 2^61).");
    std::unique_ptr<troyn_bgv, int (*)(troyn_bgv*)> b(new troyn_bgv, troyn_bgv_destroy);
    b->plan = plan; b->L = L; b->t = t;
    const std::vector<u64> q(plan->moduli.begin(), plan->moduli.begin() + L);
    std::vector<u64> inv_punc;
    if (int rc = inv_punctured(q, inv_punc)) return rc;
    ConstBlob blob;
    blob.shoup(L, element_of(inv_punc), element_of(q));
    blob.words(L, [&](size_t i) { return host::product_mod(q, i, t); });
    b->q_mod_t = host::product_mod(q, SIZE_MAX, t);
    u64 inv = 1;
    b->can_divide = host::invmod(q[L - 1] % t, t, inv);       // "[RNSTool::RNSTool] Unable to invert q[last] mod t."
    b->inv_q_last_mod_t = b->can_divide ? inv : 1;
    b->t_mod = make_dev_modulus(t, plan->log_n, false);
    if (int rc = blob.upload(plan->device, &b->d_consts)) return rc;
    *out = b.release();
    return TROYN_OK;
}

extern "C" uint64_t troyn_bgv_inv_q_last_mod_t(const troyn_bgv* b) { return b ? b->inv_q_last_mod_t : 0; }

extern "C" size_t troyn_bgv_mod_switch_workspace_bytes(const troyn_bgv* b, size_t pcount, size_t batch) {
    return b ? troyn_divide_and_round_q_last_ntt_workspace_bytes(b->plan, b->L, pcount, batch) : 0;
}

extern "C" int troyn_bgv_mod_t_and_divide_q_last_ntt(const troyn_bgv* b, const uint64_t* in, size_t pcount, uint64_t* out, void* workspace, size_t workspace_bytes,
                                                     size_t batch, troyn_stream_t stream) {
    select_device(b);
    const char* P = "[RNSTool::mod_t_and_divide_q_last_ntt]";
    if (!b || !in || !out || !workspace) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    const troyn_plan* p = b->plan;
    const unsigned L = b->L;
    if (L < 2) return fail(TROYN_E_INVALID, "[Evaluator::mod_switch_scale_to_next_internal] Next context data is not set.");
    if (!b->can_divide) return fail(TROYN_E_MODULUS, "[RNSTool::RNSTool] Unable to invert q[last] mod t.");
    if (workspace_bytes < troyn_bgv_mod_switch_workspace_bytes(b, pcount, batch)) return fail(TROYN_E_WORKSPACE, "[troyn_bgv_mod_t_and_divide_q_last_ntt] workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const size_t items = batch * pcount, n = p->n;
    if (items == 0) return TROYN_OK;
    u64* last_intt = (u64*)workspace;
    u64* delta = last_intt + items * n;
    u64* delta_ntt = delta + items * (size_t)(L - 1) * n;
    int rc;
    {   // INTT of the last limb only (the reference's device branch transforms all of them, utils/rns_tool.cu:1757)
        NttArgs a = contiguous_args(p, (const u64*)in + (size_t)(L - 1) * n, last_intt, 1, 1, L - 1, 1, TROYN_IDX_COMPONENTWISE, 0);
        a.in_bstride = (long long)L * n;
        if ((rc = launch_ntt(p, a, items, true, s))) return rc;
    }
    const unsigned ch = chunks_single(p->n);
    const size_t rows = items * (L - 1);
    if ((rc = check_rows(rows, ch))) return rc;
    hipLaunchKernelGGL(bgv_delta_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s,
                       ch, p->d_mods, L - 1, p->n, b->t_mod, b->inv_q_last_mod_t, p->moduli[L - 1], last_intt, n, delta);
    LAUNCH_CHECK();
    {
        NttArgs a = contiguous_args(p, delta, delta_ntt, 1, L - 1, 0, L - 1, TROYN_IDX_COMPONENTWISE, 0);
        if ((rc = launch_ntt(p, a, items, false, s))) return rc;
    }
    hipLaunchKernelGGL(bgv_finish_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s,
                       ch, p->d_mods, L - 1, L, p->n, (const u64*)in, delta_ntt, p->d_inv_last + (size_t)L * p->K, -1, (u64*)out, (const u64*)nullptr, (size_t)0);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_bgv_decrypt_mod_t(const troyn_bgv* b, const uint64_t* phase, uint64_t correction_factor, uint64_t* dest, size_t batch, troyn_stream_t stream) {
    select_device(b);
    const char* P = "[scaling_variant::decentralize]";
    if (!b || !phase || !dest) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (batch == 0) return TROYN_OK;
    if (batch > 65535) return fail(TROYN_E_INVALID, std::string(P) + " batch too large for one launch");
    u64 fix = 1;
    if (correction_factor != 1 && !host::invmod(correction_factor % b->t, b->t, fix)) return fail(TROYN_E_INVALID, std::string(P) + " Correction factor is not invertible.");
    BgvDecryptArgs a;
    a.mods = b->plan->d_mods;
    a.inv_punctured = reinterpret_cast<const ulonglong2*>(b->d_consts);
    a.punctured_mod_t = b->d_consts + 2 * (size_t)b->L;
    a.t = b->t_mod; a.q_mod_t = b->q_mod_t; a.fix = fix; a.L = b->L; a.n = b->plan->n;
    hipLaunchKernelGGL(bgv_decrypt_mod_t_kernel, dim3((b->plan->n + 255) / 256, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, a, (const u64*)phase, (u64*)dest);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_bgv_multiply_scalar_mod_t(const troyn_bgv* b, const uint64_t* in, uint64_t scalar, uint64_t* out, size_t count, troyn_stream_t stream) {
    select_device(b);
    if (!b || !in || !out) return fail(TROYN_E_INVALID, "[utils::multiply_scalar] null argument");
    if (count == 0) return TROYN_OK;
    hipLaunchKernelGGL(scalar_mod_t_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, b->t_mod, (u64)(scalar % b->t), (const u64*)in, (u64*)out, count);
    LAUNCH_CHECK();
    return TROYN_OK;
}

// Key switching for BGV: `key_level` = troyn_bgv_create(plan, n_moduli, t), whose last prime is the special prime
static int bgv_tail_from(const troyn_bgv* key_level, BgvTail& tail) {
    if (!key_level) return fail(TROYN_E_INVALID, "[Evaluator::switch_key_inplace_internal] null BGV constants");
    if (key_level->L != key_level->plan->K) return fail(TROYN_E_INVALID, "[Evaluator::switch_key_inplace_internal] BGV key switching needs the key level's constants");
    if (!key_level->can_divide) return fail(TROYN_E_MODULUS, "[RNSTool::RNSTool] Unable to invert q[last] mod t.");
    tail.t = key_level->t_mod; tail.inv_special_mod_t = key_level->inv_q_last_mod_t;
    return TROYN_OK;
}

extern "C" int troyn_bgv_switch_key(const troyn_bgv* key_level, uint32_t L, const uint64_t* target, const uint64_t* const* keys, int assign_method,
                                    uint64_t* destination, void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream) {
    select_device(key_level);
    BgvTail tail;
    if (int rc = bgv_tail_from(key_level, tail)) return rc;
    const troyn_plan* plan = key_level->plan;
    return switch_key_impl(plan, L, 0, 1, (const u64*)target, (size_t)L * plan->n, keys, assign_method, (u64*)destination, nullptr, 0, workspace, workspace_bytes, batch,
                           (hipStream_t)stream, &tail);
}

extern "C" int troyn_bgv_relinearize(const troyn_bgv* key_level, uint32_t L, const uint64_t* ct3, const uint64_t* const* keys, uint64_t* out2, void* workspace,
                                     size_t workspace_bytes, size_t batch, troyn_stream_t stream) {
    select_device(key_level);
    BgvTail tail;
    if (int rc = bgv_tail_from(key_level, tail)) return rc;
    if (!ct3) return fail(TROYN_E_INVALID, "[Evaluator::relinearize_inplace_internal] null argument");
    const troyn_plan* plan = key_level->plan;
    const size_t pc = (size_t)L * plan->n;
    return switch_key_impl(plan, L, 0, 1, (const u64*)ct3 + 2 * pc, 3 * pc, keys, TROYN_ASSIGN_OVERWRITE, (u64*)out2, (const u64*)ct3, 3 * pc, workspace, workspace_bytes,
                           batch, (hipStream_t)stream, &tail);
}

// ---- hoisted BGV rotations (additions; include/troyn.h, bgv_hoist_kernels.hpp): the hoisted entries' host paths in NTT form with the BGV
// division as their tail.  The handle is checked before anything else, as in troyn_bgv_switch_key ----
extern "C" int troyn_bgv_apply_galois_many(const troyn_bgv* key_level, uint32_t L, const uint64_t* ct, const uint64_t* galois_elements,
                                           const uint64_t* const* keys, size_t terms, uint64_t* out, void* workspace, size_t workspace_bytes,
                                           size_t batch, troyn_stream_t stream) {
    select_device(key_level);
    BgvTail tail;
    if (int rc = bgv_tail_from(key_level, tail)) return rc;
    return apply_galois_hoisted("[troyn_bgv_apply_galois_many]", key_level->plan, L, 0, 1, (const u64*)ct, galois_elements, keys, terms,
                                (u64*)out, workspace, workspace_bytes, batch, (hipStream_t)stream, false, &tail);
}
extern "C" int troyn_bgv_apply_galois_sum(const troyn_bgv* key_level, uint32_t L, const uint64_t* ct, const uint64_t* galois_elements,
                                          const uint64_t* const* keys, size_t terms, uint64_t* out, void* workspace, size_t workspace_bytes,
                                          size_t batch, troyn_stream_t stream) {
    select_device(key_level);
    BgvTail tail;
    if (int rc = bgv_tail_from(key_level, tail)) return rc;
    return apply_galois_hoisted("[troyn_bgv_apply_galois_sum]", key_level->plan, L, 0, 1, (const u64*)ct, galois_elements, keys, terms,
                                (u64*)out, workspace, workspace_bytes, batch, (hipStream_t)stream, true, &tail);
}
extern "C" int troyn_bgv_apply_galois_weighted_sums(const troyn_bgv* key_level, uint32_t L, const uint64_t* ct, const uint64_t* galois_elements,
                                                    const uint64_t* const* keys, size_t terms, const uint64_t* const* weights, size_t slots,
                                                    uint64_t* out, void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream) {
    select_device(key_level);
    BgvTail tail;
    if (int rc = bgv_tail_from(key_level, tail)) return rc;
    return weighted_sums_impl("[troyn_bgv_apply_galois_weighted_sums]", key_level->plan, L, 0, 1, ct, galois_elements, keys, terms, weights, slots,
                              out, workspace, workspace_bytes, batch, stream, nullptr, true, &tail);
}
extern "C" int troyn_bgv_apply_galois_sum_each(const troyn_bgv* key_level, uint32_t L, const uint64_t* cts, const uint64_t* galois_elements,
                                               const uint64_t* const* keys, size_t terms, uint64_t* out, void* workspace, size_t workspace_bytes,
                                               size_t batch, troyn_stream_t stream) {
    select_device(key_level);
    BgvTail tail;
    if (int rc = bgv_tail_from(key_level, tail)) return rc;
    const char* P = "[troyn_bgv_apply_galois_sum_each]";
    if (int rc = hoist_check_tables(P, key_level->plan, L, galois_elements, keys, terms, true)) return rc;
    return apply_galois_sum_each(P, key_level->plan, L, 0, 1, (const u64*)cts, galois_elements, keys, terms, (u64*)out,
                                 workspace, workspace_bytes, batch, (hipStream_t)stream, &tail);
}
extern "C" int troyn_bgv_linear_transform_bsgs(const troyn_bgv* key_level, uint32_t L, const uint64_t* ct,
                                               const uint64_t* baby_elements, const uint64_t* const* baby_keys, size_t babies,
                                               const uint64_t* giant_elements, const uint64_t* const* giant_keys, size_t giants,
                                               const uint64_t* const* weights, uint64_t* out,
                                               void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream) {
    select_device(key_level);
    BgvTail tail;
    if (int rc = bgv_tail_from(key_level, tail)) return rc;
    return linear_transform_bsgs_impl("[troyn_bgv_linear_transform_bsgs]", "[troyn_bgv_apply_galois_weighted_sums]", key_level->plan, L, 0, 1, ct,
                                      baby_elements, baby_keys, babies, giant_elements, giant_keys, giants, weights, out,
                                      workspace, workspace_bytes, batch, stream, &tail);
}

// ---- fused BGV chain (an addition to the reference's surface; include/troyn.h, bgv_chain_kernels.hpp) ----
// multiply -> relinearize -> mod_switch_to_next with ONE forward transform per output limb: the key switch's and the modulus switch's mod-t
// corrections are added in coefficient form.  The digit decomposition and the inner product are the key switch's own steps on c_2.
struct BgvChainLayout {
    KsLayout ks;
    size_t c2, spec, q_last, q_last_intt, delta, delta_ntt, total;      // element offsets
};
static BgvChainLayout bgv_chain_layout(const troyn_plan* p, unsigned L, size_t batch) {
    const size_t n = p->n;
    BgvChainLayout w;
    w.ks = ks_layout(p, L, batch);
    size_t off = w.ks.total;
    w.c2 = off;          off += batch * L * n;                       // a1 . b1, the key switch's target
    w.spec = off;        off += batch * 2 * n;                       // s: INTT of the special rows
    w.q_last = off;      off += batch * 2 * n;                       // Q_{L-1}
    w.q_last_intt = off; off += batch * 2 * n;
    w.delta = off;       off += batch * 2 * (size_t)(L - 1) * n;     // d_j in coefficient form
    w.delta_ntt = off;   off += batch * 2 * (size_t)(L - 1) * n;
    w.total = off;
    return w;
}

static bool bgv_chain_level_ok(const troyn_bgv* key_level, uint32_t L) {
    return key_level && key_level->plan && key_level->plan->K >= 3 && L >= 2 && L <= key_level->plan->K - 1;
}

extern "C" size_t troyn_bgv_multiply_relinearize_mod_switch_workspace_bytes(const troyn_bgv* key_level, uint32_t L, size_t batch) {
    if (!bgv_chain_level_ok(key_level, L)) return 0;
    return bgv_chain_layout(key_level->plan, L, batch).total * sizeof(u64);
}

extern "C" int troyn_bgv_multiply_relinearize_mod_switch(const troyn_bgv* key_level, const troyn_bgv* level, const uint64_t* a_, const uint64_t* b_,
                                                         const uint64_t* const* keys, uint64_t* out_, void* workspace, size_t workspace_bytes,
                                                         size_t batch, troyn_stream_t stream) {
    select_device(key_level);
    const std::string P = "[troyn_bgv_multiply_relinearize_mod_switch]";
    if (!key_level || !level || !keys) return fail(TROYN_E_INVALID, P + " null argument");
    const troyn_plan* p = key_level->plan;
    if (level->plan != p || level->t != key_level->t) return fail(TROYN_E_INVALID, P + " the two handles differ in plan or plain modulus");
    const unsigned K = p->K, n = p->n, L = level->L;
    if (K < 2) return fail(TROYN_E_INVALID, "[Evaluator::switch_key_inplace_internal] Keyswitching is not supported.");
    if (key_level->L != K) return fail(TROYN_E_INVALID, "[Evaluator::switch_key_inplace_internal] BGV key switching needs the key level's constants");
    if (L > K - 1) return fail(TROYN_E_INVALID, "[Evaluator::switch_key_inplace_internal] Invalid target size.");
    if (L < 2) return fail(TROYN_E_INVALID, "[Evaluator::mod_switch_scale_to_next_internal] Next context data is not set.");
    if (!key_level->can_divide || !level->can_divide) return fail(TROYN_E_MODULUS, "[RNSTool::RNSTool] Unable to invert q[last] mod t.");
    KeyPtrs kp;
    std::memset(&kp, 0, sizeof(kp));
    for (unsigned j = 0; j < L; j++) {
        if (!keys[j]) return fail(TROYN_E_INVALID, "[Evaluator::switch_key_inplace_internal] null key pointer");
        kp.p[j] = (const u64*)keys[j];
    }
    if (batch == 0) return TROYN_OK;
    if (!a_ || !b_ || !out_ || !workspace) return fail(TROYN_E_INVALID, P + " null argument");
    if (((uintptr_t)a_ | (uintptr_t)b_ | (uintptr_t)out_ | (uintptr_t)workspace) & 15) return fail(TROYN_E_INVALID, P + " misaligned pointer");
    const BgvChainLayout w = bgv_chain_layout(p, L, batch);
    if (workspace_bytes < w.total * sizeof(u64)) return fail(TROYN_E_WORKSPACE, P + " workspace too small");
    {   // `out` is written while a and b are still being read (the finish kernel forms c_0 and c_1 from them)
        const uintptr_t o0 = (uintptr_t)out_, o1 = o0 + batch * 2 * (size_t)(L - 1) * n * sizeof(u64);
        const size_t in_bytes = batch * 2 * (size_t)L * n * sizeof(u64);
        for (uintptr_t q : {(uintptr_t)a_, (uintptr_t)b_})
            if (q < o1 && o0 < q + in_bytes) return fail(TROYN_E_INVALID, P + " out overlaps an input");
    }
    hipStream_t s = (hipStream_t)stream;
    const u64* a = (const u64*)a_; const u64* b = (const u64*)b_;
    u64* ws = (u64*)workspace;
    const unsigned ch = chunks_pairs(n);
    int rc;
    if ((rc = check_rows(batch * 2 * (size_t)L, ch))) return rc;
    // c_2 = a1 . b1; then steps (1)-(3) of the key switch on it, on the path every BGV key switch takes
    hipLaunchKernelGGL(bgv_chain_c2_kernel, dim3((unsigned)(batch * L * ch)), dim3(POLY_BLOCK), 0, s, ch, p->d_mods, L, n, a, b, ws + w.c2);
    LAUNCH_CHECK();
    KsCall c{p, L, 0, true, ws + w.c2, (size_t)L * n, TROYN_ASSIGN_OVERWRITE, nullptr, nullptr, 0, ws, w.ks, batch, s, nullptr, ws + w.c2, (size_t)L * n};
    const KsPath path = ks_path(p, L, batch, true, true);
    if ((rc = ks_digits(c))) return rc;
    if ((rc = ks_inner_product(c, kp, path))) return rc;
    const u64* prod = ws + w.ks.poly_prod;
    const ulonglong2* inv_k = p->d_inv_last + (size_t)K * K;
    // s and INTT(Q_{L-1}): two rows per item each
    if ((rc = launch_ntt(p, special_rows_args(p, prod, ws + w.spec, L), batch, true, s))) return rc;
    hipLaunchKernelGGL(bgv_chain_last_row_kernel, dim3((unsigned)(batch * 2 * ch)), dim3(POLY_BLOCK), 0, s, ch, p->d_mods, L, n, prod, a, b, inv_k, ws + w.q_last);
    LAUNCH_CHECK();
    if ((rc = launch_ntt(p, contiguous_args(p, ws + w.q_last, ws + w.q_last_intt, 2, 1, L - 1, 1, TROYN_IDX_COMPONENTWISE, 0), batch, true, s))) return rc;
    BgvChainDeltaArgs g;
    g.mods = p->d_mods; g.inv_k = inv_k; g.t = key_level->t_mod;
    g.inv_k_mod_t = key_level->inv_q_last_mod_t; g.inv_l_mod_t = level->inv_q_last_mod_t;
    g.qk = p->moduli[K - 1]; g.ql = p->moduli[L - 1]; g.L = L; g.n = n;
    hipLaunchKernelGGL(bgv_chain_delta_kernel, dim3((unsigned)(batch * 2 * ch)), dim3(POLY_BLOCK), 0, s, ch, g, ws + w.spec, ws + w.q_last_intt, ws + w.delta);
    LAUNCH_CHECK();
    // the ONE forward transform: 2 (L-1) rows per item
    if ((rc = launch_ntt(p, contiguous_args(p, ws + w.delta, ws + w.delta_ntt, 2, L - 1, 0, L - 1, TROYN_IDX_COMPONENTWISE, 0), batch, false, s))) return rc;
    hipLaunchKernelGGL(bgv_chain_finish_kernel, dim3((unsigned)(batch * (L - 1) * ch)), dim3(POLY_BLOCK), 0, s, ch, p->d_mods, L, n, prod, a, b, ws + w.delta_ntt,
                       inv_k, p->d_inv_last + (size_t)L * K, (u64*)out_);
    LAUNCH_CHECK();
    return TROYN_OK;
}

// ---------------------------------------------------------------------------------------
// BEHZ
// ---------------------------------------------------------------------------------------
struct troyn_behz {
    const troyn_plan* plan = nullptr;   // base q (first L moduli)
    troyn_plan* aux = nullptr;          // Bsk primes (NTT tables for base Bsk, rns_tool.cu:97-101)
    unsigned L = 0, Bn = 0, Bsk = 0;
    u64 t = 0;
    std::vector<u64> bsk_values;
    u64* d_consts = nullptr;
    BehzDev dev;
    Behz2Dev dev2;                      // second-generation conversion kernels (behz2_kernels.hpp)
    bool have2 = false, smallq = false; // have2: |B| == L <= 16 and every q_i < 2^60; smallq: every q_i < 2^50
    bool aux50 = false;                 // the multiply works in an auxiliary base of primes below 2^50 (troyn_behz_create); bsk_values stays the reference's
    // encrypt / decrypt side constants of the same RNSTool / ContextData (context_data.cu:226-247, rns_tool.cu:168-211)
    u64 gamma = 0, q_mod_t = 0;
    DevModulus t_mod, gamma_mod;
    const ulonglong2* d_delta = nullptr;               // [L] floor(q/t) mod q_j
    const ulonglong2* d_prod_t_gamma_mod_q = nullptr;  // [L]
    const u64* d_q_to_t = nullptr;                     // [L]
    const u64* d_q_to_gamma = nullptr;                 // [L]
    ulonglong2 neg_inv_q_mod_t, neg_inv_q_mod_gamma, inv_gamma_mod_t;
    bool decrypt_ready = false;
    // options of the auxiliary plan = the plan's (both bases of one multiply on the same transform policies); followed at call time (below)
    mutable std::atomic<uint64_t> aux_gen{0};
    mutable std::mutex aux_mutex;
};
// A troyn_plan_set_option on the plan after troyn_behz_create used to leave base q and base Bsk on different policies inside one multiply:
// the auxiliary plan's options are brought up to date at the first call after the change (double-checked; set_option itself is a quiescent-point call).
static inline void behz_follow_options(const troyn_behz* b) {
    const uint64_t g = b->plan->opt_gen.load(std::memory_order_acquire);
    if (b->aux_gen.load(std::memory_order_acquire) == g || !b->aux) return;
    std::lock_guard<std::mutex> lock(b->aux_mutex);
    if (b->aux_gen.load(std::memory_order_relaxed) == g) return;
    b->aux->opt = b->plan->opt;
    b->aux_gen.store(g, std::memory_order_release);
}

extern "C" int troyn_behz_destroy(troyn_behz* b) {
    if (!b) return TROYN_OK;
    if (b->aux) plan_free(b->aux);
    if (b->d_consts) (void)hipFree(b->d_consts);
    delete b;
    return TROYN_OK;
}

static const u64 BEHZ_M_TILDE = (u64)1 << 32;

// troyn_behz_create, step by step
struct BehzBase {
    std::vector<u64> B, bsk;      // the base the multiply works in, and B + {m_sk}
    u64 m_sk = 0;
    bool aux50 = false;           // B and m_sk are primes below 2^50
};

// The working base.  BEHZ's result does not depend on the auxiliary primes: the conversion q -> Bsk yields the integer x + alpha q
// (alpha < L, a function of the residues mod q only), the small Montgomery reduction works modulo m_tilde = 2^32, the floor is an exact
// integer division in base Bsk and the Shenoy-Kumaresan conversion back to q is exact as long as the value fits B -- all statements about
// integers, true for ANY base whose product is at least the reference's (utils/rns_tool.cu:52-80 sizes B as |q| or |q| + 1 primes of 61 bits).
// When every q_i is below 2^50 the 61-bit base is the only reason half of the multiply's transforms, its tensor product and its two
// conversions run on the integer butterflies (27.5 issue slots against 8 FP64 instructions): take instead NB primes BELOW 2^50 with
//     prod(B') >= 2^(61 Bn)   and   prod(B') m_sk' >= 2^(61 (Bn + 1)),
// i.e. at least the capacity of any base the reference could have picked, so that every transform of the multiply takes the exact-FP64
// policy.  The oracle keeps the reference's base; equality of the final residues on every BEHZ test is the proof.
// MEASURED (round 4, BASELINE config 4, profiles/r04_cfg4_ab.txt): bit-identical results, and no gain -- the tensor kernels drop from 1.33 to
// 1.01 ms per 64 products, but 13 + 1 primes instead of 10 + 1 make both conversions 29 % longer (0.66 -> 0.83 ms for the floor alone) and
// add three limbs to every strided pass: 14.0 k against 14.2 k mul+relin ops/s.  ROUND 5: 13 + 1 came from asking for the capacity of the
// reference's base itself; the reference's own size criterion (below) is met by 11 + 1 primes -- one row more than the 61-bit base instead of
// three: tensor launches 1.33 -> 0.95 ms per 64 products, 14.15 k -> 14.7 k ops/s same box.  It is the DEFAULT whenever it applies (every q_i
// below 2^50, second-generation conversions); TROYN_BEHZ_BASE=ref keeps the reference's base (read here).
static int behz_choose_base(troyn_behz* b, const std::vector<u64>& q, BehzBase& base) {
    const troyn_plan* plan = b->plan;
    // auxiliary base sizes and primes: utils/rns_tool.cu:52-80
    const size_t L = q.size();
    size_t Bn = L;
    if (32 + host::bit_count(b->t) + host::product_bit_count(q) >= 61 * L + 61) Bn++;
    std::vector<u64> primes, fresh;
    try {
        primes = host::get_primes(2 * (u64)plan->n, 61, Bn + 2);
    } catch (const std::exception& e) {
        return fail(TROYN_E_MODULUS, e.what());
    }
    base.m_sk = primes[0];
    b->gamma = primes[1];         // decrypt side only
    base.B.assign(primes.begin() + 2, primes.begin() + 2 + Bn);
    b->bsk_values = base.B; b->bsk_values.push_back(base.m_sk);      // the reference's base (troyn_behz_get_base_Bsk: known-answer hook), whatever base the multiply works in
    base.aux50 = !plan->opt.behz_base_ref && !plan->opt.behz_v1 && L <= BEHZ2_MAX_L && plan->log_n >= 10;
    for (u64 v : q) if (v >= F64_MODULUS_LIMIT) base.aux50 = false;
    if (base.aux50) try {
        for (u64 c : host::get_primes(2 * (u64)plan->n, 50, plan->K + 2 * (Bn + 1) + 8))
            if (std::find(plan->moduli.begin(), plan->moduli.end(), c) == plan->moduli.end()) fresh.push_back(c);
    } catch (const std::exception&) { fresh.clear(); }
    // Size of the base: the reference's own criterion (utils/rns_tool.cu:50-62: K n t q^2 < q prod(B) m_sk with 32 bits reserved for K n, i.e.
    // bits(prod(B) m_sk) > 32 + bits(t) + bits(q); it states it for 61-bit primes as 61 (#B + 1)) evaluated on the ACTUAL product of the primes
    // taken, with two more bits of margin.  (Round 4 asked for the capacity of the reference's base itself, 2^(61 (Bn + 1)): 13 + 1 primes at
    // BASELINE config 4 where 11 + 1 satisfy the criterion -- every conversion and strided pass scales with the number of rows.)
    const size_t need_bits = 32 + (size_t)host::product_bit_count(std::vector<u64>{b->t}) + (size_t)host::product_bit_count(q) + 2;
    auto enough = [&](const std::vector<u64>& B) {
        std::vector<u64> with_sk = B; with_sk.push_back(fresh[0]);      // fresh[0] becomes m_sk'
        return (size_t)host::product_bit_count(with_sk) > need_bits;
    };
    std::vector<u64> B2;
    for (size_t next = 1; next < fresh.size(); next++) {
        B2.push_back(fresh[next]);
        if (enough(B2)) break;
    }
    base.aux50 = !B2.empty() && enough(B2) && B2.size() <= 32;
    if (base.aux50) { base.B = B2; base.m_sk = fresh[0]; }
    base.bsk = base.B; base.bsk.push_back(base.m_sk);
    // Shenoy-Kumaresan (rns_tool.cu:1000-1036): the correction term alpha_sk of the conversion B -> q is recovered modulo m_sk and satisfies
    // |alpha_sk| <= |B| (+ the lambda of the fast floor); it is read off a centred residue, so m_sk must exceed twice that -- any prime of 50 or
    // 61 bits does by ~45 bits, but the working base is chosen above, so state what it relies on
    if (base.m_sk < 2 * ((u64)base.B.size() + 2) + 1) return fail(TROYN_E_MODULUS, "[troyn_behz_create] m_sk is too small for the Shenoy-Kumaresan correction of this base");
    b->Bn = (unsigned)base.B.size(); b->Bsk = (unsigned)base.bsk.size(); b->aux50 = base.aux50;
    return TROYN_OK;
}

// the auxiliary plan: NTT tables of the working base; it takes the options its plan has now and follows later changes (behz_follow_options)
static int behz_create_aux_plan(troyn_behz* b, const troyn_plan* plan, const BehzBase& base) {
    const int rc = troyn_plan_create(&b->aux, plan->device, plan->log_n, (uint32_t)base.bsk.size(), reinterpret_cast<const uint64_t*>(base.bsk.data()), nullptr);
    if (rc != TROYN_OK) return rc;
    b->aux->opt = plan->opt;
    b->aux_gen.store(plan->opt_gen.load(std::memory_order_acquire), std::memory_order_release);
    return TROYN_OK;
}

// multiply side (first-generation kernels; the second generation shares q_mt_inv_punc and q_t_inv_punc)
static int behz_multiply_tables(troyn_behz* b, const std::vector<u64>& q, const BehzBase& base, ConstBlob& blob) {
    const std::vector<u64>& B = base.B;
    const std::vector<u64>& bsk = base.bsk;
    const size_t L = q.size(), Bn = B.size(), Bsk = bsk.size();
    const u64 mt = BEHZ_M_TILDE, m_sk = base.m_sk, t = b->t;
    BehzDev& d = b->dev;
    auto q_of = element_of(q), bsk_of = element_of(bsk);
    // every inverse once
    std::vector<u64> q_inv, B_inv, prod_q(Bsk), inv_mt(Bsk), inv_prod_q(Bsk);
    if (int rc = inv_punctured(q, q_inv)) return rc;
    for (size_t bi = 0; bi < Bsk; bi++) prod_q[bi] = host::product_mod(q, SIZE_MAX, bsk[bi]);
    for (size_t bi = 0; bi < Bsk; bi++)
        if (!host::invmod(mt % bsk[bi], bsk[bi], inv_mt[bi])) return fail(TROYN_E_MODULUS, "[RNSTool::RNSTool] Unable to invert m_tilde.");
    for (size_t bi = 0; bi < Bsk; bi++)
        if (!host::invmod(prod_q[bi] % bsk[bi], bsk[bi], inv_prod_q[bi])) return fail(TROYN_E_MODULUS, "[RNSTool::RNSTool] Unable to invert base_q product.");
    if (int rc = inv_punctured(B, B_inv)) return rc;
    blob.bind(&d.q_inv_punc, blob.shoup(L, element_of(q_inv), q_of));
    // the scalar factor that precedes a base conversion folded into its first step: (x * c mod q_i) * inv_punc_i mod q_i
    // = x * (c * inv_punc_i mod q_i) mod q_i -- one Shoup multiply instead of a Barrett-128 product followed by one (c = m_tilde for
    // the lift, evaluator.cu:52-56 + rns_tool.cu:1083-1094; c = t for the floor, evaluator.cu:95-100)
    blob.bind(&d.q_mt_inv_punc, blob.shoup(L, [&](size_t i) { return host::mulmod(mt % q[i], q_inv[i], q[i]); }, q_of));
    blob.bind(&d.q_t_inv_punc, blob.shoup(L, [&](size_t i) { return host::mulmod(t % q[i], q_inv[i], q[i]); }, q_of));
    blob.bind(&d.q_to_bsk, blob.words(Bsk * L, [&](size_t k) { return host::product_mod(q, k % L, bsk[k / L]); }));
    blob.bind(&d.q_to_mt, blob.words(L, [&](size_t i) { return host::product_mod(q, i, mt); }));
    blob.bind(&d.prod_q_mod_bsk, blob.shoup(Bsk, element_of(prod_q), bsk_of));
    blob.bind(&d.inv_mt_mod_bsk, blob.shoup(Bsk, element_of(inv_mt), bsk_of));
    blob.bind(&d.inv_prod_q_mod_bsk, blob.shoup(Bsk, element_of(inv_prod_q), bsk_of));
    // (x * t - f) * q^-1 = x * (t q^-1) - f * q^-1 mod p_b: the floor's multiplication by t folded into the division by q
    blob.bind(&d.t_inv_prod_q_mod_bsk, blob.shoup(Bsk, [&](size_t bi) { return host::mulmod(t % bsk[bi], inv_prod_q[bi], bsk[bi]); }, bsk_of));
    blob.bind(&d.B_inv_punc, blob.shoup(Bn, element_of(B_inv), element_of(B)));
    blob.bind(&d.B_to_q, blob.words(L * Bn, [&](size_t k) { return host::product_mod(B, k % Bn, q[k / Bn]); }));
    blob.bind(&d.B_to_msk, blob.words(Bn, [&](size_t bi) { return host::product_mod(B, bi, m_sk); }));
    blob.bind(&d.prod_B_mod_q, blob.shoup(L, [&](size_t i) { return host::product_mod(B, SIZE_MAX, q[i]); }, q_of));
    blob.bind(&d.neg_prod_B_mod_q, blob.shoup(L, [&](size_t i) { return q[i] - host::product_mod(B, SIZE_MAX, q[i]); }, q_of));
    u64 inv;
    if (!host::invmod(host::product_mod(q, SIZE_MAX, mt) % mt, mt, inv)) return fail(TROYN_E_MODULUS, "[RNSTool::RNSTool] Unable to invert base_q product.");
    d.neg_inv_prod_q_mod_mt = shoup_pair(mt - inv, mt);
    if (!host::invmod(host::product_mod(B, SIZE_MAX, m_sk) % m_sk, m_sk, inv)) return fail(TROYN_E_MODULUS, "[RNSTool::RNSTool] Unable to invert base_B product.");
    d.inv_prod_B_mod_msk = shoup_pair(inv, m_sk);
    return TROYN_OK;
}

// second-generation conversion tables (split matrices with the scalar factors folded in); sets have2 / smallq
static void behz_second_generation_tables(troyn_behz* b, const std::vector<u64>& q, const BehzBase& base, ConstBlob& blob) {
    Behz2Offsets o;
    Behz2Dev& e = b->dev2;
    b->have2 = (base.B.size() == q.size() || base.aux50) && q.size() <= BEHZ2_MAX_L;
    b->smallq = true;
    for (u64 v : q) { if (v >> 60) b->have2 = false; if (v >= F64_MODULUS_LIMIT) b->smallq = false; }
    if (b->have2) b->have2 = behz2_build_tables(q, base.B, base.m_sk, b->t, b->smallq, blob.aligned(), o);
    if (!b->have2) return;
    e.rs = o.rs;
    blob.bind(&e.lift_mt, o.lift_mt); blob.bind(&e.lift_rows, o.lift_rows); blob.bind(&e.lift_rc, o.lift_rc);
    blob.bind(&e.fa_rows, o.fa_rows); blob.bind(&e.fa_rc, o.fa_rc);
    blob.bind(&e.fb_cols, o.fb_cols); blob.bind(&e.fb_rc, o.fb_rc);
}

// encrypt / decrypt side: constants of the same RNSTool / ContextData (context_data.cu:226-247, rns_tool.cu:168-211)
static void behz_decrypt_tables(troyn_behz* b, const std::vector<u64>& q, ConstBlob& blob) {
    const u64 t = b->t, gamma = b->gamma;
    const size_t L = q.size();
    auto q_of = element_of(q);
    std::vector<u64> q_over_t = host::big_product(q);       // floor(q / t) as a multi-word integer
    b->q_mod_t = host::big_divmod_small(q_over_t, t);
    blob.bind(&b->d_delta, blob.shoup(L, [&](size_t i) { return host::big_mod_small(q_over_t, q[i]); }, q_of));
    blob.bind(&b->d_prod_t_gamma_mod_q, blob.shoup(L, [&](size_t i) { return host::mulmod(t % q[i], gamma % q[i], q[i]); }, q_of));
    blob.bind(&b->d_q_to_t, blob.words(L, [&](size_t i) { return host::product_mod(q, i, t); }));
    blob.bind(&b->d_q_to_gamma, blob.words(L, [&](size_t i) { return host::product_mod(q, i, gamma); }));
    u64 inv_gamma = 0, inv_q_t = 0, inv_q_gamma = 0;
    b->decrypt_ready = host::invmod(gamma % t, t, inv_gamma);                // "[RNSTool::RNSTool] Unable to invert gamma mod t."
    b->decrypt_ready &= host::invmod(host::product_mod(q, SIZE_MAX, t) % t, t, inv_q_t);
    b->decrypt_ready &= host::invmod(host::product_mod(q, SIZE_MAX, gamma) % gamma, gamma, inv_q_gamma);
    b->inv_gamma_mod_t = shoup_pair(inv_gamma, t);
    b->neg_inv_q_mod_t = shoup_pair(t - inv_q_t, t);
    b->neg_inv_q_mod_gamma = shoup_pair(gamma - inv_q_gamma, gamma);
    b->t_mod = make_dev_modulus(t, b->plan->log_n, false);
    b->gamma_mod = make_dev_modulus(gamma, b->plan->log_n, false);
}

// what the kernels' argument blocks hold besides the table rows (those were bound where they were built)
static void behz_wire(troyn_behz* b) {
    const troyn_plan* plan = b->plan;
    BehzDev& d = b->dev;
    d.L = b->L; d.Bn = b->Bn; d.Bsk = b->Bsk; d.n = plan->n; d.t = b->t;
    d.q_mods = plan->d_mods; d.bsk_mods = b->aux->d_mods;
    d.m_tilde = make_dev_modulus(BEHZ_M_TILDE, plan->log_n, false);
    if (!b->have2) return;
    Behz2Dev& e = b->dev2;
    e.L = b->L; e.n = plan->n; e.NB = b->Bn;
    e.q_mods = plan->d_mods; e.q_mt_inv_punc = d.q_mt_inv_punc; e.q_t_inv_punc = d.q_t_inv_punc;
}

extern "C" int troyn_behz_create(troyn_behz** out, const troyn_plan* plan, uint32_t L, uint64_t t) {
    if (!out || !plan) return fail(TROYN_E_INVALID, "[troyn_behz_create] null argument");
    *out = nullptr;
    if (L < 1 || L > plan->K) return fail(TROYN_E_INVALID, "[RNSTool::RNSTool] RNSBase length is invalid.");
    if (t == 0 || (t >> 61) != 0 || t == 1) return fail(TROYN_E_MODULUS, "[troyn_behz_create] BFV needs a plain modulus in [2, 2^61).");
    std::unique_ptr<troyn_behz, int (*)(troyn_behz*)> b(new troyn_behz, troyn_behz_destroy);
    b->plan = plan; b->L = L; b->t = t;
    std::memset(&b->dev, 0, sizeof(b->dev));
    std::memset(&b->dev2, 0, sizeof(b->dev2));
    const std::vector<u64> q(plan->moduli.begin(), plan->moduli.begin() + L);
    BehzBase base;
    ConstBlob blob;              // all tables in one allocation
    if (int rc = behz_choose_base(b.get(), q, base)) return rc;
    if (int rc = behz_create_aux_plan(b.get(), plan, base)) return rc;
    if (int rc = behz_multiply_tables(b.get(), q, base, blob)) return rc;
    behz_second_generation_tables(b.get(), q, base, blob);
    behz_decrypt_tables(b.get(), q, blob);
    if (int rc = blob.upload(plan->device, &b->d_consts)) return rc;
    behz_wire(b.get());
    *out = b.release();
    return TROYN_OK;
}

extern "C" uint32_t troyn_behz_base_Bsk_size(const troyn_behz* b) { return b ? (uint32_t)b->bsk_values.size() : 0; }
extern "C" uint32_t troyn_behz_working_base_size(const troyn_behz* b) { return b ? b->Bsk : 0; }
extern "C" int troyn_behz_get_base_Bsk(const troyn_behz* b, uint64_t* out) {
    select_device(b);
    if (!b || !out) return fail(TROYN_E_INVALID, "[troyn_behz_get_base_Bsk] null argument");
    for (size_t i = 0; i < b->bsk_values.size(); i++) out[i] = b->bsk_values[i];
    return TROYN_OK;
}

struct BehzLayout { size_t a_q, a_bsk, b_q, b_bsk, d_q, d_bsk, total; };
static BehzLayout behz_layout(const troyn_behz* b, size_t pa, size_t pb, size_t batch) {
    const size_t n = b->plan->n, L = b->L, S = b->Bsk, po = pa + pb - 1;
    BehzLayout w; size_t off = 0;
    w.a_q = off;   off += batch * pa * L * n;
    w.a_bsk = off; off += batch * pa * S * n;
    w.b_q = off;   off += batch * pb * L * n;
    w.b_bsk = off; off += batch * pb * S * n;
    w.d_q = off;   off += batch * po * L * n;
    w.d_bsk = off; off += batch * po * S * n;
    w.total = off;
    return w;
}

extern "C" size_t troyn_bfv_multiply_workspace_bytes(const troyn_behz* b, size_t pa, size_t pb, size_t batch) {
    if (!b || pa < 1 || pb < 1) return 0;
    return behz_layout(b, pa, pb, batch).total * sizeof(u64);
}

// first-generation kernels: instantiated per bound on the row count
static void launch_behz1_lift(const troyn_behz* b, dim3 grid, hipStream_t s, unsigned ch1, const u64* src, u64* dst_bsk) {
    auto* kernel = b->L <= 4 ? behz_lift_kernel<4> : b->L <= 8 ? behz_lift_kernel<8> : b->L <= 16 ? behz_lift_kernel<16> : behz_lift_kernel<64>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, ch1, b->dev, src, dst_bsk);
}
static void launch_behz1_floor(const troyn_behz* b, dim3 grid, hipStream_t s, unsigned ch1, const u64* d_q, const u64* d_bsk, u64* out) {
    auto* kernel = b->Bsk <= 4 ? behz_floor_kernel<4> : b->Bsk <= 8 ? behz_floor_kernel<8> : b->Bsk <= 16 ? behz_floor_kernel<16> : behz_floor_kernel<66>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, ch1, b->dev, d_q, d_bsk, out);
}

// one validated call: base q on plan pq (L limbs), the working base on plan px (S limbs)
struct BfvCall {
    const troyn_behz* b; const troyn_plan* pq; const troyn_plan* px; unsigned L, S;
    const u64* a; size_t pa;
    const u64* bb; size_t pb;
    u64* out; u64* ws; BehzLayout w; size_t batch; hipStream_t s;
};

// which launches one multiply takes: decided once per call
struct BfvPath {
    int tkind;          // tensor_path_kind of both bases when they agree and the operands have two components: 1 whole-limb tiles, 2 two-pass sizes; 0: no tensor kernel
    bool lift_fused;    // N = 32768: the lift inside the first forward pass, the last inverse pass inside the floor
    bool gen2;          // second-generation conversion kernels
    bool square;        // a ciphertext multiplied with itself: one lift, and the staged copies of b are those of a
    bool tensor() const { return tkind != 0; }
    bool whole() const { return tkind == 1; }
};
static BfvPath bfv_path(const BfvCall& c) {
    const troyn_plan* pq = c.pq;
    const troyn_plan* px = c.px;
    const unsigned L = c.L, S = c.S;
    BfvPath k;
    k.gen2 = c.b->have2 && !pq->opt.behz_v1;   // TROYN_BEHZ=v1: first-generation kernels (A/B runs and the tests of that path)
    // 2 x 2 components at a two-pass size: the forward transforms stop after their first pass, tensor_core_kernel finishes them, forms the
    // product and starts the inverse transforms
    k.tkind = (c.pa == 2 && c.pb == 2 && tensor_path_kind(pq, L) == tensor_path_kind(px, S)) ? tensor_path_kind(pq, L) : 0;
    // Whole-limb sizes, a few ciphertexts: tensor_core_kernel puts seven transforms of a limb on ONE workgroup (L + S workgroups per item) -- a launch
    // that cannot fill the chip is one long chain (one product at N = 16384 6 x 50-bit: 240 us).  The separate launches (two-pass transforms of many
    // small workgroups, dyadic product) finish in 92 us (N = 8192 {60,40,40,60}: 245 -> 78 us for one product).  TROYN_BFV_TENSOR=fused / split force either.
    // (the hand-over point, measured: ~200 workgroups where tensor_core_kernel is at its best -- N <= 8192, FP64 policy -- and ~350 where it spills
    // (N = 16384) or runs the integer butterflies)
    const size_t tensor_small = (pq->log_n <= 13 && use_f64(pq, 0, L) && use_f64(px, 0, S)) ? 192 : 352;
    if (k.tkind == 1 && !pq->opt.tensor_fused && c.batch * (size_t)(L + S) <= tensor_small) k.tkind = 0;
    // N = 32768 under the FP64 policy: first pass of base q, lift and first pass of the lifted rows as one launch, and the last inverse pass of
    // both bases inside the floor launch (behz2_lift_pass1.hpp)
    k.lift_fused = k.tkind == 2 && k.gen2 && c.b->aux50 && c.b->smallq && pq->log_n == 15 && !pq->opt.behz_lift_split
                   && use_f64(pq, 0, L) && use_f64(px, 0, S) && L + S <= BEHZ2_FUSED_MAX_ROWS;
    k.square = c.a == c.bb && c.pa == c.pb;
    return k;
}

// steps (1)-(3) of evaluator.cu:50-60 for one operand
static int bfv_lift(const BfvCall& c, const BfvPath& path, const u64* src, size_t pcount, u64* dst_q, u64* dst_bsk) {
    const troyn_behz* b = c.b;
    const size_t items = c.batch * pcount;
    if (path.lift_fused) {
        if (items * 512u > 0x7fffffffull) return fail(TROYN_E_INVALID, "[troyn_bfv_multiply] batch too large for one launch");
        // (lift_fused holds only for shapes both fused launches cover: the floor skips the last inverse pass on the same condition)
        if (!launch_behz2_lift_pass1(c.L, items, c.s, b->dev2, src, dst_q, dst_bsk, (const double*)c.pq->d_fwd_f64, (const double*)c.px->d_fwd_f64, c.pq->d_mods, c.px->d_mods))
            return fail(TROYN_E_INVALID, "[troyn_bfv_multiply] no fused lift kernel for this shape");
        LAUNCH_CHECK();
        return TROYN_OK;
    }
    // the forward transform of one base; whole-limb tiles: none, the tensor kernel reads coefficient form
    auto forward = [&](const troyn_plan* p, const u64* in, u64* dst, unsigned nc) {
        NttArgs a = contiguous_args(p, in, dst, pcount, nc, 0, nc, TROYN_IDX_COMPONENTWISE, 0);
        return path.whole() ? TROYN_OK : path.tensor() ? tensor_stage(p, 0, a, a, a, c.batch, c.s) : launch_ntt(p, a, c.batch, false, c.s);
    };
    const unsigned ch1 = chunks_single(c.pq->n);
    if (int rc = forward(c.pq, src, dst_q, c.L)) return rc;
    if (int rc = check_rows(items, ch1)) return rc;
    dim3 grid((unsigned)(items * ch1));
    if (path.gen2) launch_behz2_lift(c.L, b->smallq, grid.x, c.s, ch1, b->dev2, src, dst_bsk, b->aux50);
    else launch_behz1_lift(b, grid, c.s, ch1, src, dst_bsk);
    LAUNCH_CHECK();
    return forward(c.px, dst_bsk, dst_bsk, c.S);
}

// steps (4)-(5), 2 x 2 components: tensor_core_kernel per base
static int bfv_tensor(const BfvCall& c, const BfvPath& path) {
    const BehzLayout& w = c.w;
    for (int base = 0; base < 2; base++) {
        const troyn_plan* p = base ? c.px : c.pq;
        const unsigned nc = base ? c.S : c.L;
        // whole-limb tiles: base q is read straight from the operands (coefficient form), nothing of it is staged
        const u64* xa = (path.whole() && !base) ? c.a : c.ws + (base ? w.a_bsk : w.a_q);
        const u64* xb = (path.whole() && !base) ? c.bb : c.ws + (base ? w.b_bsk : w.b_q);
        u64* xd = c.ws + (base ? w.d_bsk : w.d_q);
        NttArgs fa = contiguous_args(p, xa, nullptr, 2, nc, 0, nc, TROYN_IDX_COMPONENTWISE, 0);
        NttArgs fb = contiguous_args(p, xb, nullptr, 2, nc, 0, nc, TROYN_IDX_COMPONENTWISE, 0);
        NttArgs id = contiguous_args(p, xd, xd, 3, nc, 0, nc, TROYN_IDX_COMPONENTWISE, 0);
        {
            TimerScope ts(TROYN_TIMER_BFV_TENSOR, c.s);
            if (int rc = tensor_stage(p, 1, fa, fb, id, c.batch, c.s)) return rc;
        }
        if (!path.whole() && !path.lift_fused)      // lift_fused: the floor launch runs the last pass
            if (int rc = tensor_stage(p, 2, id, id, id, c.batch, c.s)) return rc;
    }
    return TROYN_OK;
}

// steps (4)-(5), any component counts: dyadic convolution and inverse transforms per base
static int bfv_convolute_intt(const BfvCall& c) {
    const BehzLayout& w = c.w;
    const size_t po = c.pa + c.pb - 1;
    u64* ws = c.ws;
    if (int rc = launch_convolute(c.pq->d_mods, c.pq->n, 0, c.L, ws + w.a_q, c.pa, ws + w.b_q, c.pb, ws + w.d_q, c.batch, c.s)) return rc;
    if (int rc = launch_convolute(c.px->d_mods, c.pq->n, 0, c.S, ws + w.a_bsk, c.pa, ws + w.b_bsk, c.pb, ws + w.d_bsk, c.batch, c.s)) return rc;
    NttArgs a = contiguous_args(c.pq, ws + w.d_q, ws + w.d_q, po, c.L, 0, c.L, TROYN_IDX_COMPONENTWISE, 0);
    if (int rc = launch_ntt(c.pq, a, c.batch, true, c.s)) return rc;
    NttArgs ab = contiguous_args(c.px, ws + w.d_bsk, ws + w.d_bsk, po, c.S, 0, c.S, TROYN_IDX_COMPONENTWISE, 0);
    return launch_ntt(c.px, ab, c.batch, true, c.s);
}

// steps (6)-(8)
static int bfv_floor(const BfvCall& c, const BfvPath& path) {
    const troyn_behz* b = c.b;
    const unsigned ch1 = chunks_single(c.pq->n);
    const u64* d_q = c.ws + c.w.d_q;
    const u64* d_bsk = c.ws + c.w.d_bsk;
    const size_t items = c.batch * (c.pa + c.pb - 1);
    if (int rc = check_rows(items, ch1)) return rc;
    dim3 grid((unsigned)(items * ch1));
    TimerScope ts(TROYN_TIMER_BEHZ_FLOOR, c.s);
    if (path.lift_fused) {
        if (items * 512u > 0x7fffffffull) return fail(TROYN_E_INVALID, "[troyn_bfv_multiply] batch too large for one launch");
        if (!launch_behz2_floor_pass2(c.L, items, c.s, b->dev2, d_q, d_bsk, c.out, (const double*)c.pq->d_inv_f64, (const double*)c.px->d_inv_f64, c.pq->d_mods, c.px->d_mods))
            return fail(TROYN_E_INVALID, "[troyn_bfv_multiply] no fused floor kernel for this shape");
    } else if (path.gen2) {
        launch_behz2_floor(c.L, b->smallq, grid.x, c.s, ch1, b->dev2, d_q, d_bsk, c.out, b->aux50);
    } else launch_behz1_floor(b, grid, c.s, ch1, d_q, d_bsk, c.out);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_bfv_multiply(const troyn_behz* b, const uint64_t* a_, size_t pa, const uint64_t* b_, size_t pb,
                                  uint64_t* out, void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream) {
    select_device(b);
    if (!b || !a_ || !b_ || !out || !workspace) return fail(TROYN_E_INVALID, "[Evaluator::bfv_multiply_inplace] null argument");
    if (pa < 1 || pb < 1 || pa > 16 || pb > 16) return fail(TROYN_E_INVALID, "[Evaluator::bfv_multiply_inplace] invalid ciphertext size");
    const BehzLayout w = behz_layout(b, pa, pb, batch);
    if (workspace_bytes < w.total * sizeof(u64)) return fail(TROYN_E_WORKSPACE, "[troyn_bfv_multiply] workspace too small");
    if (batch == 0) return TROYN_OK;
    behz_follow_options(b);
    BfvCall c{b, b->plan, b->aux, b->L, b->Bsk, (const u64*)a_, pa, (const u64*)b_, pb, (u64*)out, (u64*)workspace, w, batch, (hipStream_t)stream};
    const BfvPath path = bfv_path(c);
    if (path.square) { c.w.b_q = w.a_q; c.w.b_bsk = w.a_bsk; }
    if (int rc = bfv_lift(c, path, c.a, pa, c.ws + w.a_q, c.ws + w.a_bsk)) return rc;
    if (!path.square) if (int rc = bfv_lift(c, path, c.bb, pb, c.ws + w.b_q, c.ws + w.b_bsk)) return rc;
    if (int rc = path.tensor() ? bfv_tensor(c, path) : bfv_convolute_intt(c)) return rc;
    return bfv_floor(c, path);
}

// ---- BFV inner product: SUM_t lift(a[t]) (x) lift(b[t]) in NTT form over both bases, ONE inverse tensor pass, floor and conversion ----
// (additions to the reference's surface, include/troyn.h).  Every step between the lift and the floor is linear modulo each prime, so the
// words are those of the per-pair products summed as integers before the floor -- as long as the sum fits the auxiliary base:
//     T N t q (1 + rho)^2 < prod(B) m_sk,     (1 + rho)^2 < 2  (rho = 2 L / m_tilde, m_tilde = 2^32).
// The reference's base has prod(B) m_sk > 2^(61 (#B + 1) - 1) >= 2^(32 + bits(t) + bits(q)) > 2^32 t q (its primes are the largest below
// 2^61), behz_choose_base's working base > 2^(34 + bits(t) + bits(q)): T N < 2^31 holds in either.  The cap of 1024 terms gives
// T N <= 2^27 at N = 2^17, four bits to spare.
constexpr size_t BFV_ACC_MAX_TERMS = 1024;
constexpr size_t BFV_ACC_CHUNK = TENSOR_ACC_MAX_TERMS;      // terms lifted and accumulated at a time (the kernel's pointer table)
static_assert(BFV_ACC_CHUNK == 32, "include/troyn.h states the chunk");

// workspace: stage_q / stage_bsk: 2 * chunk lifted operands (every distinct pointer of a chunk is lifted once) | d_q, d_bsk: the sum
// | [prod3: the floor's output | the key switch's own workspace]
struct BfvAccLayout { BehzLayout w; size_t slots, slot_q, slot_bsk, prod3, sub, sub_bytes, total_bytes; };
static BfvAccLayout bfv_acc_layout(const troyn_behz* b, size_t terms, size_t batch, bool relin) {
    const size_t n = b->plan->n, L = b->L, S = b->Bsk;
    BfvAccLayout y;
    y.slots = 2 * std::min(terms, BFV_ACC_CHUNK);
    y.slot_q = batch * 2 * L * n; y.slot_bsk = batch * 2 * S * n;
    size_t off = 0;
    y.w.a_q = y.w.b_q = off;     off += y.slots * y.slot_q;
    y.w.a_bsk = y.w.b_bsk = off; off += y.slots * y.slot_bsk;
    y.w.d_q = off;   off += batch * 3 * L * n;
    y.w.d_bsk = off; off += batch * 3 * S * n;
    y.w.total = off;
    y.prod3 = off; if (relin) off += batch * 3 * L * n;
    y.sub = off;
    y.sub_bytes = relin ? troyn_relinearize_workspace_bytes(b->plan, (uint32_t)L, batch) : 0;
    y.total_bytes = off * sizeof(u64) + y.sub_bytes;
    return y;
}

// one chunk of staged terms into d (one base): tensor_accumulate_kernel
static int bfv_tensor_accumulate(const troyn_plan* p, unsigned nc, const u64* const* xa, const u64* const* xb, unsigned cnt, u64* d, bool carry, size_t batch, hipStream_t s) {
    TensorAccPtrs g;
    for (unsigned t = 0; t < (unsigned)TENSOR_ACC_MAX_TERMS; t++) { g.a[t] = xa[t < cnt ? t : 0]; g.b[t] = xb[t < cnt ? t : 0]; }
    NttArgs fa = contiguous_args(p, xa[0], nullptr, 2, nc, 0, nc, TROYN_IDX_COMPONENTWISE, 0);
    NttArgs id = contiguous_args(p, d, d, 3, nc, 0, nc, TROYN_IDX_COMPONENTWISE, 0);
    prep_direct(p, fa, true, false); prep_direct(p, id, true, true);
    if (carry) id.flags |= NTT_FLAG_MID_CARRY;
    if ((batch * 3 * nc) << (p->log_n - 12) > 0x7fffffffull) return fail(TROYN_E_INVALID, "[troyn_bfv_multiply_accumulate] batch too large for one launch");
    if (!launch_tensor_accumulate(p->log_n, true, fa, g, cnt, id, batch, launch_ctx(p, s)))
        return fail(TROYN_E_INVALID, "[troyn_bfv_multiply_accumulate] no accumulating tensor kernel for this size");
    LAUNCH_CHECK();
    return TROYN_OK;
}

// the sum into out3 [batch][3][L][N] (arguments checked by the entries)
static int bfv_accumulate(const troyn_behz* b, const uint64_t* const* a, const uint64_t* const* bb, size_t terms, u64* out3, u64* ws,
                          const BfvAccLayout& y, size_t batch, hipStream_t s) {
    behz_follow_options(b);
    BfvCall c{b, b->plan, b->aux, b->L, b->Bsk, (const u64*)a[0], 2, (const u64*)bb[0], 2, out3, ws, y.w, batch, s};
    BfvPath path = bfv_path(c);
    // The accumulating kernel exists for the two-pass sizes and the FP64 class.  Whole-limb sizes (tensor_core_kernel is at its register
    // cap there), limbs of the integer class, TROYN_BFV_TENSOR=split and the small rings: full forward transforms into the staging area,
    // dyadic_convolute_accumulate_kernel per base, inverse transforms.
    if (path.tkind != 2 || !use_f64(c.pq, 0, c.L) || !use_f64(c.px, 0, c.S)) { path.tkind = 0; path.lift_fused = false; }
    const u64* src[2 * BFV_ACC_CHUNK];
    const u64* xa_q[BFV_ACC_CHUNK]; const u64* xb_q[BFV_ACC_CHUNK]; const u64* xa_x[BFV_ACC_CHUNK]; const u64* xb_x[BFV_ACC_CHUNK];
    auto tab = [](const u64* const* x) { return reinterpret_cast<const uint64_t* const*>(x); };
    u64* const stage_q = ws + y.w.a_q;
    u64* const stage_x = ws + y.w.a_bsk;
    for (size_t t0 = 0; t0 < terms; t0 += BFV_ACC_CHUNK) {
        const unsigned cnt = (unsigned)std::min(terms - t0, BFV_ACC_CHUNK);
        size_t used = 0;
        // steps (1)-(3) once per distinct operand of the chunk (a[t] == b[t], one ciphertext in several terms)
        auto staged = [&](const u64* ptr, size_t& slot) -> int {
            for (slot = 0; slot < used; slot++) if (src[slot] == ptr) return TROYN_OK;
            src[used++] = ptr;
            return bfv_lift(c, path, ptr, 2, stage_q + slot * y.slot_q, stage_x + slot * y.slot_bsk);
        };
        for (unsigned t = 0; t < cnt; t++) {
            size_t sa, sb;
            if (int rc = staged((const u64*)a[t0 + t], sa)) return rc;
            if (int rc = staged((const u64*)bb[t0 + t], sb)) return rc;
            xa_q[t] = stage_q + sa * y.slot_q; xa_x[t] = stage_x + sa * y.slot_bsk;
            xb_q[t] = stage_q + sb * y.slot_q; xb_x[t] = stage_x + sb * y.slot_bsk;
        }
        const bool carry = t0 > 0;
        TimerScope ts(TROYN_TIMER_BFV_TENSOR, s);
        if (path.tensor()) {
            if (int rc = bfv_tensor_accumulate(c.pq, c.L, xa_q, xb_q, cnt, ws + y.w.d_q, carry, batch, s)) return rc;
            if (int rc = bfv_tensor_accumulate(c.px, c.S, xa_x, xb_x, cnt, ws + y.w.d_bsk, carry, batch, s)) return rc;
        } else {
            if (int rc = launch_convolute_accumulate(c.pq->d_mods, c.pq->n, 0, c.L, tab(xa_q), tab(xb_q), cnt, ws + y.w.d_q, carry, batch, s)) return rc;
            if (int rc = launch_convolute_accumulate(c.px->d_mods, c.pq->n, 0, c.S, tab(xa_x), tab(xb_x), cnt, ws + y.w.d_bsk, carry, batch, s)) return rc;
        }
    }
    // the last inverse pass (lift_fused: inside the floor launch) or the inverse transforms, once
    for (int base = 0; base < 2; base++) {
        const troyn_plan* p = base ? c.px : c.pq;
        const unsigned nc = base ? c.S : c.L;
        u64* xd = ws + (base ? y.w.d_bsk : y.w.d_q);
        NttArgs id = contiguous_args(p, xd, xd, 3, nc, 0, nc, TROYN_IDX_COMPONENTWISE, 0);
        if (path.tensor()) { if (!path.lift_fused) if (int rc = tensor_stage(p, 2, id, id, id, batch, s)) return rc; }
        else if (int rc = launch_ntt(p, id, batch, true, s)) return rc;
    }
    return bfv_floor(c, path);
}

// checks shared by the two entries; out_words: size of `out`
static int bfv_accumulate_check(const char* P, const troyn_behz* b, const uint64_t* const* a, const uint64_t* const* bb, size_t terms,
                                const uint64_t* out, size_t out_words, size_t batch) {
    if (!b || !a || !bb) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (terms > BFV_ACC_MAX_TERMS) return fail(TROYN_E_INVALID, std::string(P) + " more than 1024 terms");
    return check_convolute_accumulate(P, b->plan, 0, b->L, a, bb, terms, out, out_words, batch);
}

extern "C" size_t troyn_bfv_multiply_accumulate_workspace_bytes(const troyn_behz* b, size_t terms, size_t batch) {
    if (!b || terms == 0 || terms > BFV_ACC_MAX_TERMS) return 0;
    return bfv_acc_layout(b, terms, batch, false).total_bytes;
}

extern "C" int troyn_bfv_multiply_accumulate(const troyn_behz* b, const uint64_t* const* a, const uint64_t* const* bb, size_t terms,
                                             uint64_t* out, void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream) {
    select_device(b);
    const char* P = "[troyn_bfv_multiply_accumulate]";
    if (int rc = bfv_accumulate_check(P, b, a, bb, terms, out, batch * 3 * (size_t)(b ? b->L : 0) * (b ? b->plan->n : 0), batch)) return rc;
    if (batch == 0) return TROYN_OK;
    const BfvAccLayout y = bfv_acc_layout(b, terms, batch, false);
    if (!workspace || workspace_bytes < y.total_bytes) return fail(TROYN_E_WORKSPACE, std::string(P) + " workspace too small");
    if ((uintptr_t)workspace & 15) return fail(TROYN_E_INVALID, std::string(P) + " misaligned workspace");
    return bfv_accumulate(b, a, bb, terms, (u64*)out, (u64*)workspace, y, batch, (hipStream_t)stream);
}

extern "C" size_t troyn_bfv_multiply_accumulate_relinearize_workspace_bytes(const troyn_behz* b, size_t terms, size_t batch) {
    if (!b || terms == 0 || terms > BFV_ACC_MAX_TERMS) return 0;
    return bfv_acc_layout(b, terms, batch, true).total_bytes;
}

extern "C" int troyn_bfv_multiply_accumulate_relinearize(const troyn_behz* b, const uint64_t* const* a, const uint64_t* const* bb, size_t terms,
                                                         const uint64_t* const* keys, uint64_t* out, void* workspace, size_t workspace_bytes,
                                                         size_t batch, troyn_stream_t stream) {
    select_device(b);
    const char* P = "[troyn_bfv_multiply_accumulate_relinearize]";
    if (!keys) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (int rc = bfv_accumulate_check(P, b, a, bb, terms, out, batch * 2 * (size_t)(b ? b->L : 0) * (b ? b->plan->n : 0), batch)) return rc;
    if (batch == 0) return TROYN_OK;
    const BfvAccLayout y = bfv_acc_layout(b, terms, batch, true);
    if (!workspace || workspace_bytes < y.total_bytes) return fail(TROYN_E_WORKSPACE, std::string(P) + " workspace too small");
    if ((uintptr_t)workspace & 15) return fail(TROYN_E_INVALID, std::string(P) + " misaligned workspace");
    u64* ws = (u64*)workspace;
    if (int rc = bfv_accumulate(b, a, bb, terms, ws + y.prod3, ws, y, batch, (hipStream_t)stream)) return rc;
    // Evaluator::relinearize on coefficient-form BFV data (evaluator_keyswitching.cu:119-144): one key switch for the whole sum
    return troyn_relinearize(b->plan, b->L, 0, 0, (const uint64_t*)(ws + y.prod3), keys, out, ws + y.sub, y.sub_bytes, batch, stream);
}

// ---------------------------------------------------------------------------------------
// context PRNG samplers, BFV plaintext scaling, BFV decryption rounding
// ---------------------------------------------------------------------------------------
extern "C" int troyn_prng_block(const uint64_t seed[2], uint64_t counter, uint64_t out[2]) {
    if (!seed || !out) return fail(TROYN_E_INVALID, "[troyn_prng_block] null argument");
    const AesRoundKeys k = aes128_expand(seed[0], seed[1]);
    u64 lo, hi;
    aes128_encrypt_counter(k, counter, 0, lo, hi);
    out[0] = lo; out[1] = hi;
    return TROYN_OK;
}

template <typename K>
static int launch_sampler(K kernel, const char* who, const troyn_plan* p, uint32_t nmod, const uint64_t seed[2], uint64_t counter,
                          uint64_t* out, size_t blocks, uint64_t* blocks_used, troyn_stream_t stream, size_t threads = 0) {
    if (!p || !seed || !out) return fail(TROYN_E_INVALID, std::string(who) + " null argument");
    if (nmod == 0 || nmod > p->K) return fail(TROYN_E_INVALID, std::string(who) + " modulus count out of range");
    const AesRoundKeys k = aes128_expand(seed[0], seed[1]);
    if (!threads) threads = blocks;        // one thread per AES block unless the kernel says otherwise
    hipLaunchKernelGGL(kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       k, (u64)counter, p->d_mods, (unsigned)nmod, p->n, (u64*)out);
    LAUNCH_CHECK();
    if (blocks_used) *blocks_used = blocks;
    return TROYN_OK;
}

extern "C" int troyn_sample_ternary(const troyn_plan* p, uint32_t nmod, const uint64_t seed[2], uint64_t counter, uint64_t* out,
                                    uint64_t* blocks_used, troyn_stream_t stream) {
    select_device(p);
    return launch_sampler(sample_ternary_kernel, "[RandomGenerator::sample_poly_ternary]", p, nmod, seed, counter, out,
                          p ? ((size_t)p->n + 15) / 16 : 0, blocks_used, stream, p ? (size_t)p->n : 0);      // (a thread per coefficient)
}
// fixed Hamming weight: one workgroup selects the h smallest of N keyed words in place, row 0 of `out` staging the keys
extern "C" int troyn_sample_ternary_sparse(const troyn_plan* p, uint32_t nmod, const uint64_t seed[2], uint64_t counter, uint32_t hamming_weight,
                                           uint64_t* out, uint64_t* blocks_used, troyn_stream_t stream) {
    select_device(p);
    const char* P = "[RandomGenerator::sample_poly_ternary_sparse]";
    if (!p || !seed || !out) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (nmod == 0 || nmod > p->K) return fail(TROYN_E_INVALID, std::string(P) + " modulus count out of range");
    if (hamming_weight == 0 || hamming_weight > p->n) return fail(TROYN_E_INVALID, std::string(P) + " hamming weight must be in [1, N]");
    if (p->n < 2 || p->n > 65536) return fail(TROYN_E_INVALID, std::string(P) + " the 16-bit index of a key needs N <= 65536");
    if ((uintptr_t)out & 15) return fail(TROYN_E_INVALID, std::string(P) + " misaligned destination");
    const AesRoundKeys k = aes128_expand(seed[0], seed[1]);
    hipLaunchKernelGGL(sample_ternary_sparse_kernel, dim3(1), dim3(SPARSE_TERNARY_THREADS), 0, (hipStream_t)stream,
                       k, (u64)counter, p->d_mods, (unsigned)nmod, p->n, (unsigned)hamming_weight, (u64*)out);
    LAUNCH_CHECK();
    if (blocks_used) *blocks_used = p->n / 2;
    return TROYN_OK;
}
extern "C" int troyn_sample_centered_binomial(const troyn_plan* p, uint32_t nmod, const uint64_t seed[2], uint64_t counter, uint64_t* out,
                                              uint64_t* blocks_used, troyn_stream_t stream) {
    select_device(p);
    return launch_sampler(sample_cbd_kernel, "[RandomGenerator::sample_poly_centered_binomial]", p, nmod, seed, counter, out,
                          p ? ((size_t)p->n + 1) / 2 : 0, blocks_used, stream);
}
extern "C" int troyn_sample_uniform(const troyn_plan* p, uint32_t nmod, const uint64_t seed[2], uint64_t counter, uint64_t* out,
                                    uint64_t* blocks_used, troyn_stream_t stream) {
    select_device(p);
    return launch_sampler(sample_uniform_kernel, "[RandomGenerator::sample_poly_uniform]", p, nmod, seed, counter, out,
                          p ? ((size_t)p->n * nmod + 1) / 2 : 0, blocks_used, stream);
}

extern "C" int troyn_sample_centered_binomial_strided(const troyn_plan* p, uint32_t nmod, const uint64_t seed[2], uint64_t counter, uint64_t counter_stride,
                                                      uint64_t* out, size_t count, troyn_stream_t stream) {
    select_device(p);
    const char* P = "[RandomGenerator::sample_poly_centered_binomial]";
    if (!p || !seed || !out) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (nmod == 0 || nmod > p->K) return fail(TROYN_E_INVALID, std::string(P) + " modulus count out of range");
    if (count == 0) return TROYN_OK;
    if (count > 65535) return fail(TROYN_E_INVALID, std::string(P) + " batch too large for one launch");
    const AesRoundKeys k = aes128_expand(seed[0], seed[1]);
    const unsigned blocks = (unsigned)((((size_t)p->n + 1) / 2 + 255) / 256);
    hipLaunchKernelGGL(sample_cbd_strided_kernel, dim3(blocks, (unsigned)count), dim3(256), 0, (hipStream_t)stream,
                       k, (u64)counter, (u64)counter_stride, p->d_mods, (unsigned)nmod, p->n, (u64*)out);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_sample_uniform_multi(const troyn_plan* p, uint32_t nmod, const uint64_t* seeds, uint64_t* out, size_t count, troyn_stream_t stream) {
    select_device(p);
    const char* P = "[RandomGenerator::sample_poly_uniform]";
    if (!p || !seeds || !out) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (nmod == 0 || nmod > p->K) return fail(TROYN_E_INVALID, std::string(P) + " modulus count out of range");
    const size_t per_item = (size_t)nmod * p->n;
    const unsigned blocks = (unsigned)(((per_item + 1) / 2 + 255) / 256);
    for (size_t base = 0; base < count; base += SAMPLE_MULTI_KEYS) {
        const size_t m = std::min<size_t>(SAMPLE_MULTI_KEYS, count - base);
        AesRoundKeysMulti keys;
        std::memset(&keys, 0, sizeof(keys));
        for (size_t i = 0; i < m; i++) keys.k[i] = aes128_expand(seeds[2 * (base + i)], seeds[2 * (base + i) + 1]);
        hipLaunchKernelGGL(sample_uniform_multi_kernel, dim3(blocks, (unsigned)m), dim3(256), 0, (hipStream_t)stream,
                           keys, p->d_mods, (unsigned)nmod, p->n, (u64*)out + base * per_item);
        LAUNCH_CHECK();
    }
    return TROYN_OK;
}

extern "C" int troyn_bfv_scale_up(const troyn_behz* b, const uint64_t* plain, size_t plain_coeff_count, size_t plain_bstride,
                                  const uint64_t* from, size_t from_bstride, uint64_t* dest, size_t dest_bstride,
                                  int subtract, size_t batch, troyn_stream_t stream) {
    select_device(b);
    if (!b || !plain || !dest) return fail(TROYN_E_INVALID, "[scaling_variant::scale_up] null argument");
    const unsigned n = b->plan->n;
    if (plain_coeff_count > n) return fail(TROYN_E_INVALID, "[scaling_variant::scale_up] destination_coeff_count should no less than plain_coeff_count.");
    if (batch == 0) return TROYN_OK;
    ScaleUpArgs a;
    std::memset(&a, 0, sizeof(a));
    a.L = b->L; a.n = n; a.plain_coeff_count = (unsigned)plain_coeff_count; a.subtract = subtract ? 1u : 0u;
    a.mods = b->plan->d_mods; a.delta = b->d_delta; a.t = b->t_mod; a.q_mod_t = b->q_mod_t; a.threshold = (b->t + 1) >> 1;
    a.plain = (const u64*)plain; a.plain_bstride = (long long)plain_bstride;
    a.from = (const u64*)from; a.from_bstride = (long long)from_bstride;
    a.dest = (u64*)dest; a.dest_bstride = (long long)dest_bstride;
    const unsigned ch = chunks_single(n);
    const size_t rows = batch * b->L;
    if (int rc = check_rows(rows, ch)) return rc;
    hipLaunchKernelGGL(bfv_scale_up_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, (hipStream_t)stream, ch, a);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_bfv_decrypt_scale_and_round(const troyn_behz* b, const uint64_t* phase, uint64_t* dest, size_t batch, troyn_stream_t stream) {
    select_device(b);
    if (!b || !phase || !dest) return fail(TROYN_E_INVALID, "[RNSTool::decrypt_scale_and_round] null argument");
    if (!b->decrypt_ready) return fail(TROYN_E_MODULUS, "[RNSTool::RNSTool] Unable to invert gamma mod t.");
    if (batch == 0) return TROYN_OK;
    DecryptArgs c;
    std::memset(&c, 0, sizeof(c));
    c.L = b->L; c.n = b->plan->n; c.mods = b->plan->d_mods; c.t = b->t_mod; c.gamma = b->gamma_mod;
    c.prod_t_gamma_mod_q = b->d_prod_t_gamma_mod_q; c.q_inv_punc = b->dev.q_inv_punc;
    c.q_to_t = b->d_q_to_t; c.q_to_gamma = b->d_q_to_gamma;
    c.neg_inv_q_mod_t = b->neg_inv_q_mod_t; c.neg_inv_q_mod_gamma = b->neg_inv_q_mod_gamma; c.inv_gamma_mod_t = b->inv_gamma_mod_t;
    const unsigned ch = chunks_single(c.n);
    if (int rc = check_rows(batch, ch)) return rc;
    hipLaunchKernelGGL(bfv_decrypt_round_kernel, dim3((unsigned)(batch * ch)), dim3(256), 0, (hipStream_t)stream, ch, c, (const u64*)phase, (u64*)dest);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" uint64_t troyn_behz_gamma(const troyn_behz* b) { return b ? b->gamma : 0; }

// ---------------------------------------------------------------------------------------
// ciphertext x plaintext
// ---------------------------------------------------------------------------------------
extern "C" int troyn_plain_centralize(const troyn_plan* p, uint32_t L, uint64_t t, const uint64_t* plain, size_t plain_coeff_count,
                                      size_t plain_bstride, uint64_t* dest, size_t batch, troyn_stream_t stream) {
    select_device(p);
    if (!p || !plain || !dest) return fail(TROYN_E_INVALID, "[scaling_variant::centralize] null argument");
    if (L < 1 || L > p->K) return fail(TROYN_E_INVALID, "[scaling_variant::centralize] Destination has incorrect size.");
    if (plain_coeff_count > p->n) return fail(TROYN_E_INVALID, "[scaling_variant::centralize] destination_coeff_count should no less than plain_coeff_count.");
    if (batch == 0) return TROYN_OK;
    const unsigned ch = chunks_single(p->n);
    const size_t rows = batch * L;
    if (int rc = check_rows(rows, ch)) return rc;
    hipLaunchKernelGGL(plain_centralize_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, (hipStream_t)stream,
                       ch, p->d_mods, (unsigned)L, p->n, (u64)t, (const u64*)plain, (unsigned)plain_coeff_count, (long long)plain_bstride, (u64*)dest);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_plain_centralize_ntt(const troyn_plan* p, uint32_t L, uint64_t t, const uint64_t* plain, size_t plain_coeff_count,
                                          size_t plain_bstride, uint64_t* dest, size_t batch, troyn_stream_t stream) {
    select_device(p);
    if (!p || !plain || !dest) return fail(TROYN_E_INVALID, "[Evaluator::transform_plain_to_ntt] null argument");
    if (L < 1 || L > p->K) return fail(TROYN_E_INVALID, "[scaling_variant::centralize] Destination has incorrect size.");
    if (plain_coeff_count > p->n) return fail(TROYN_E_INVALID, "[scaling_variant::centralize] destination_coeff_count should no less than plain_coeff_count.");
    if (batch == 0) return TROYN_OK;
    bool fast = p->log_n >= 10 && t >= 2;
    for (uint32_t j = 0; fast && j < L; j++) fast = t < p->moduli[j];
    if (!fast) {
        // the general lift (t not below every q_j) and the rings the optimised transforms do not cover: the two launches
        if (int rc = troyn_plain_centralize(p, L, t, plain, plain_coeff_count, plain_bstride, dest, batch, stream)) return rc;
        return troyn_ntt(p, 0, dest, dest, batch, 1, L, 0, L, TROYN_IDX_COMPONENTWISE, 0, stream);
    }
    // one forward launch whose loader reads the plaintext row (shared by the L limbs: component stride 0, the limbs of an item co-located on an XCD)
    NttArgs a = contiguous_args(p, (const u64*)plain, (u64*)dest, 1, L, 0, L, TROYN_IDX_COMPONENTWISE, 0);
    a.in_cstride = 0; a.in_pstride = 0; a.in_bstride = (long long)plain_bstride;
    a.load_mode = NTT_LOAD_CENTRALIZE; a.cz_t = t; a.cz_count = (unsigned)plain_coeff_count;
    return launch_ntt(p, a, batch, false, (hipStream_t)stream);
}

extern "C" int troyn_dyadic_broadcast_product(const troyn_plan* p, uint32_t mod_start, uint32_t nmod, const uint64_t* ct, size_t pcount,
                                              const uint64_t* pt, size_t pt_bstride, uint64_t* out, size_t batch, troyn_stream_t stream) {
    select_device(p);
    if (!p || !ct || !pt || !out) return fail(TROYN_E_INVALID, "[dyadic_product_ps] null argument");
    if (nmod == 0 || mod_start + nmod > p->K) return fail(TROYN_E_INVALID, "[dyadic_product_ps] modulus slice out of range");
    if (batch == 0 || pcount == 0) return TROYN_OK;
    const unsigned ch = chunks_pairs(p->n);
    const size_t rows = batch * nmod;
    if (int rc = check_rows(rows, ch)) return rc;
    hipLaunchKernelGGL(dyadic_broadcast_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, (hipStream_t)stream,
                       ch, p->d_mods, mod_start, nmod, p->n, (unsigned)pcount, (const u64*)ct, (const u64*)pt, (long long)pt_bstride, (u64*)out);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_apply_galois(const troyn_plan* p, uint32_t mod_start, uint32_t nmod, int is_ntt_form, uint64_t galois_element,
                                  const uint64_t* in, uint64_t* out, size_t count, troyn_stream_t stream) {
    select_device(p);
    if (!p || !in || !out) return fail(TROYN_E_INVALID, "[GaloisTool::apply] null argument");
    if (in == out) return fail(TROYN_E_INVALID, "[GaloisTool::apply] the permutation cannot run in place");
    if (nmod == 0 || mod_start + nmod > p->K) return fail(TROYN_E_INVALID, "[GaloisTool::apply] modulus slice out of range");
    if ((galois_element & 1) == 0 || galois_element >= 2ull * p->n) return fail(TROYN_E_INVALID, "[Evaluator::apply_galois_inplace] Galois element is not valid.");
    if (p->log_n < 1) return fail(TROYN_E_INVALID, "[GaloisTool::GaloisTool] coeff_count_power is invalid");
    const size_t rows = count * nmod;
    if (rows == 0) return TROYN_OK;
    const unsigned ch = chunks_single(p->n);
    if (int rc = check_rows(rows, ch)) return rc;
    hipLaunchKernelGGL(galois_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, (hipStream_t)stream,
                       ch, p->d_mods, mod_start, nmod, p->log_n, (unsigned)galois_element, is_ntt_form ? 1 : 0, (const u64*)in, (u64*)out, (u64)0);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_apply_galois_plain(const troyn_plan* p, uint64_t modulus, uint64_t galois_element, const uint64_t* in, uint64_t* out, size_t count,
                                        troyn_stream_t stream) {
    select_device(p);
    if (!p || !in || !out) return fail(TROYN_E_INVALID, "[GaloisTool::apply] null argument");
    if (in == out) return fail(TROYN_E_INVALID, "[GaloisTool::apply] the permutation cannot run in place");
    if (modulus < 2) return fail(TROYN_E_INVALID, "[GaloisTool::apply] modulus is invalid");
    if ((galois_element & 1) == 0 || galois_element >= 2ull * p->n) return fail(TROYN_E_INVALID, "[Evaluator::apply_galois_inplace] Galois element is not valid.");
    if (count == 0) return TROYN_OK;
    const unsigned ch = chunks_single(p->n);
    if (int rc = check_rows(count, ch)) return rc;
    hipLaunchKernelGGL(galois_kernel, dim3((unsigned)(count * ch)), dim3(POLY_BLOCK), 0, (hipStream_t)stream,
                       ch, p->d_mods, 0u, 1u, p->log_n, (unsigned)galois_element, 0, (const u64*)in, (u64*)out, (u64)modulus);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_negacyclic_shift(const troyn_plan* p, uint32_t mod_start, uint32_t nmod, const uint64_t* in, uint64_t* out, size_t shift,
                                      size_t count, troyn_stream_t stream) {
    select_device(p);
    const char* P = "[negacyclic_shift_ps]";
    if (!p || !in || !out) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (in == out) return fail(TROYN_E_INVALID, std::string(P) + " the shift cannot run in place");
    if (nmod == 0 || mod_start + nmod > p->K) return fail(TROYN_E_INVALID, std::string(P) + " modulus slice out of range");
    shift %= 2ull * p->n;      // the reference takes any shift: index (shift + k) & (N - 1), sign from bit log2 N of shift + k (utils/poly_small_mod.cu:927-944)
    const size_t rows = count * nmod;
    if (rows == 0) return TROYN_OK;
    const unsigned ch = chunks_single(p->n);
    if (int rc = check_rows(rows, ch)) return rc;
    hipLaunchKernelGGL(negacyclic_shift_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, (hipStream_t)stream,
                       ch, p->d_mods, mod_start, nmod, p->log_n, (unsigned)shift, (const u64*)in, (u64*)out);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_multiply_inv_degree(const troyn_plan* p, uint32_t mod_start, uint32_t nmod, const uint64_t* in, uint64_t* out, uint64_t scalar,
                                         size_t count, troyn_stream_t stream) {
    select_device(p);
    const char* P = "[ntt_multiply_inv_degree]";
    if (!p || !in || !out) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (nmod == 0 || mod_start + nmod > p->K) return fail(TROYN_E_INVALID, std::string(P) + " modulus slice out of range");
    const size_t rows = count * nmod;
    if (rows == 0) return TROYN_OK;
    const unsigned ch = chunks_single(p->n);
    if (int rc = check_rows(rows, ch)) return rc;
    hipLaunchKernelGGL(multiply_inv_degree_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, (hipStream_t)stream,
                       ch, p->d_mods, mod_start, nmod, p->n, (u64)scalar, (const u64*)in, (u64*)out);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" size_t troyn_pack_prepare_workspace_bytes(size_t slots) { return (slots + 1) * sizeof(u64); }

extern "C" int troyn_pack_prepare(const troyn_plan* p, uint32_t L, size_t pcount, const uint64_t* const* src, size_t slots, uint64_t mul, size_t shift,
                                  uint64_t* out, void* workspace, size_t workspace_bytes, troyn_stream_t stream) {
    select_device(p);
    const char* P = "[Evaluator::pack_rlwe_ciphertexts_new]";
    if (!p || !src || !out || !workspace) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (L == 0 || L > p->K) return fail(TROYN_E_INVALID, std::string(P) + " modulus count out of range");
    shift %= 2ull * p->n;      // the reference takes any shift: index (shift + k) & (N - 1), sign from bit log2 N of shift + k (utils/poly_small_mod.cu:927-944)
    if (slots == 0 || pcount == 0) return TROYN_OK;
    if (workspace_bytes < troyn_pack_prepare_workspace_bytes(slots)) return fail(TROYN_E_WORKSPACE, "[troyn_pack_prepare] workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = upload_host_table(s, workspace, src, slots * sizeof(u64))) return rc;
    const size_t rows = slots * pcount * L;
    const unsigned ch = chunks_single(p->n);
    if (int rc = check_rows(rows, ch)) return rc;
    hipLaunchKernelGGL(pack_prepare_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s,
                       ch, p->d_mods, (unsigned)L, p->log_n, (unsigned)pcount, (u64)mul, (unsigned)shift, (const u64* const*)workspace, (u64*)out);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_pack_layer(const troyn_plan* p, uint32_t L, uint64_t galois_element, size_t shift, const uint64_t* in, uint64_t* out,
                                uint64_t* target, size_t pairs, troyn_stream_t stream) {
    select_device(p);
    const char* P = "[Evaluator::pack_rlwe_ciphertexts_new]";
    if (!p || !in || !out || !target) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (L == 0 || L > p->K) return fail(TROYN_E_INVALID, std::string(P) + " modulus count out of range");
    if ((galois_element & 1) == 0 || galois_element >= 2ull * p->n) return fail(TROYN_E_INVALID, "[Evaluator::apply_galois_inplace] Galois element is not valid.");
    shift %= 2ull * p->n;      // the reference takes any shift: index (shift + k) & (N - 1), sign from bit log2 N of shift + k (utils/poly_small_mod.cu:927-944)
    if (pairs == 0) return TROYN_OK;
    // g^-1 mod 2N (g odd): Newton iteration on the 2-adic inverse
    const u64 two_n = 2ull * p->n;
    u64 inv = galois_element;
    for (int it = 0; it < 6; it++) inv = inv * (2 - galois_element * inv);
    inv &= two_n - 1;
    const size_t rows = pairs * 2 * L;
    const unsigned ch = chunks_single(p->n);
    if (int rc = check_rows(rows, ch)) return rc;
    hipLaunchKernelGGL(pack_layer_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, (hipStream_t)stream,
                       ch, p->d_mods, (unsigned)L, p->log_n, (unsigned)shift, (unsigned)inv, (const u64*)in, (u64*)out, (u64*)target);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" size_t troyn_extract_lwe_workspace_bytes(size_t count) { return (count + (count + 1) / 2 + 1) * sizeof(u64); }

extern "C" int troyn_extract_lwe(const troyn_plan* p, uint32_t L, const uint64_t* const* ct, const size_t* terms, uint64_t* c0, uint64_t* c1, size_t count,
                                 void* workspace, size_t workspace_bytes, troyn_stream_t stream) {
    select_device(p);
    const char* P = "[Evaluator::extract_lwe_new]";
    if (!p || !ct || !terms || !c0 || !c1 || !workspace) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (L == 0 || L > p->K) return fail(TROYN_E_INVALID, std::string(P) + " modulus count out of range");
    if (count == 0) return TROYN_OK;
    if (count * L > 0x7fffffffull) return fail(TROYN_E_INVALID, std::string(P) + " batch too large for one launch");
    if (workspace_bytes < troyn_extract_lwe_workspace_bytes(count)) return fail(TROYN_E_WORKSPACE, "[troyn_extract_lwe] workspace too small");
    const size_t n = p->n, pc = (size_t)L * n;
    std::vector<u64> tab(count + (count + 1) / 2, 0);
    unsigned* t32 = reinterpret_cast<unsigned*>(tab.data() + count);
    for (size_t i = 0; i < count; i++) {
        if (!ct[i]) return fail(TROYN_E_INVALID, std::string(P) + " null pointer in the batch");
        if (terms[i] >= n) return fail(TROYN_E_INVALID, std::string(P) + " term out of range");
        tab[i] = (u64)(uintptr_t)ct[i];
        t32[i] = (unsigned)terms[i];
    }
    hipStream_t s = (hipStream_t)stream;
    if (int rc = upload_host_table(s, workspace, tab.data(), tab.size() * sizeof(u64))) return rc;
    // c1 of the LWE = c1 of the RLWE shifted by 2N - term (term 0: unshifted), evaluator_lwes.cu:72-79
    const unsigned ch = chunks_single(p->n);
    for (size_t i = 0; i < count; i++) {
        const size_t shift = terms[i] == 0 ? 0 : 2 * n - terms[i];
        hipLaunchKernelGGL(negacyclic_shift_kernel, dim3((unsigned)(L * ch)), dim3(POLY_BLOCK), 0, s,
                           ch, p->d_mods, 0u, (unsigned)L, p->log_n, (unsigned)shift, (const u64*)ct[i] + pc, (u64*)c1 + i * pc);
    }
    hipLaunchKernelGGL(extract_lwe_c0_kernel, dim3((unsigned)((count * L + 255) / 256)), dim3(256), 0, s,
                       (unsigned)L, (unsigned)n, (const u64* const*)workspace, (const unsigned*)((const u64*)workspace + count), (u64*)c0, (unsigned)count);
    LAUNCH_CHECK();
    return TROYN_OK;
}

// ---------------------------------------------------------------------------------------
// ring-2^k encoder (src/app/bfv_ring2k.cu): constants of PolynomialEncoderRNSHelper for one level
// ---------------------------------------------------------------------------------------
struct troyn_ring2k {
    const troyn_plan* plan = nullptr;
    u64* d_consts = nullptr;
    Ring2kDev dev;
    u64 gamma = 0;
};

extern "C" int troyn_ring2k_destroy(troyn_ring2k* h) {
    if (!h) return TROYN_OK;
    if (h->d_consts) (void)hipFree(h->d_consts);
    delete h;
    return TROYN_OK;
}

extern "C" int troyn_ring2k_create(troyn_ring2k** out, const troyn_plan* plan, uint32_t L, uint32_t t_bits, uint32_t elem_bytes) {
    const char* P = "[PolynomialEncoderRNSHelper::PolynomialEncoderRNSHelper]";
    if (!out || !plan) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    *out = nullptr;
    if (L < 1 || L > plan->K) return fail(TROYN_E_INVALID, std::string(P) + " modulus count out of range");
    if (elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 16) return fail(TROYN_E_INVALID, std::string(P) + " T must be uint32_t, uint64_t or uint128_t");
    if (t_bits <= elem_bytes * 4 || t_bits > elem_bytes * 8) return fail(TROYN_E_INVALID, std::string(P) + " t_bit_length must be greater than type_bits<T>() / 2");
    typedef unsigned __int128 u128h;
    std::unique_ptr<troyn_ring2k, int (*)(troyn_ring2k*)> h(new troyn_ring2k, troyn_ring2k_destroy);
    h->plan = plan;
    const std::vector<u64> q(plan->moduli.begin(), plan->moduli.begin() + L);
    u64 gamma;
    try { gamma = host::get_primes((u64)plan->n, 61, 1)[0]; } catch (const std::exception& e) { return fail(TROYN_E_MODULUS, e.what()); }
    for (u64 v : q) if (v == gamma) return fail(TROYN_E_MODULUS, std::string(P) + " gamma is in coeff_modulus");
    h->gamma = gamma;
    const u128h mask = t_bits == 128 ? ~(u128h)0 : (((u128h)1 << t_bits) - 1);
    auto wrap_product = [&](size_t except) { u128h acc = 1; for (size_t k = 0; k < q.size(); k++) if (k != except) acc *= q[k]; return acc; };   // mod 2^128
    auto inverse_2k = [](u128h x) { u128h inv = x; for (int it = 0; it < 8; it++) inv *= 2 - x * inv; return inv; };                            // x odd
    const u128h Q128 = wrap_product(SIZE_MAX);
    const u128h q_mod_t = Q128 & mask, neg_inv_q = (0 - inverse_2k(Q128)) & mask, inv_gamma = inverse_2k((u128h)gamma) & mask, t_half = (u128h)1 << (t_bits - 1);
    // floor(Q / 2^k) mod q_l from the multi-word product
    std::vector<u64> big = host::big_product(q), shifted(big.size(), 0);
    for (size_t w = 0; w < big.size(); w++) {
        const size_t src = w + t_bits / 64;
        u64 v = src < big.size() ? big[src] >> (t_bits % 64) : 0;
        if ((t_bits % 64) && src + 1 < big.size()) v |= big[src + 1] << (64 - t_bits % 64);
        shifted[w] = v;
    }
    Ring2kDev& d = h->dev;
    std::memset(&d, 0, sizeof(d));
    ConstBlob blob;
    blob.bind(&d.q_div_t_mod_q, blob.shoup(L, [&](size_t l) { return host::big_mod_small(shifted, q[l]); }, element_of(q)));
    blob.bind(&d.gamma_t_mod_q, blob.shoup(L, [&](size_t l) {
        // gamma * 2^k mod q_l, with 2^k split as 2^(k/2) * 2^(k - k/2) (bfv_ring2k.cu:183-191)
        const u64 t0 = (u64)(((u128h)1 << (t_bits / 2)) % q[l]), t1 = (u64)(((u128h)1 << (t_bits - t_bits / 2)) % q[l]);
        return host::mulmod(gamma % q[l], host::mulmod(t0, t1, q[l]), q[l]);
    }, element_of(q)));
    std::vector<u64> inv_punc;
    if (int rc = inv_punctured(q, inv_punc)) return rc;
    blob.bind(&d.inv_punctured, blob.shoup(L, element_of(inv_punc), element_of(q)));
    blob.bind(&d.punctured_mod_gamma, blob.words(L, [&](size_t l) { return host::product_mod(q, l, gamma); }));
    blob.aligned();                                                            // [L] 128-bit values, low word first
    blob.bind(&d.punctured_mod_t, blob.words(2 * (size_t)L, [&](size_t k) { return (u64)((wrap_product(k / 2) & mask) >> (64 * (k % 2))); }));
    u64 inv_q_gamma = 0;
    if (!host::invmod(host::product_mod(q, SIZE_MAX, gamma), gamma, inv_q_gamma)) return fail(TROYN_E_MODULUS, std::string(P) + " failed to invert Q_mod_gamma");
    if (int rc = blob.upload(plan->device, &h->d_consts)) return rc;
    d.mods = plan->d_mods;
    d.gamma = make_dev_modulus(gamma, plan->log_n, false);
    d.neg_inv_q_mod_gamma = shoup_pair(gamma - inv_q_gamma, gamma);
    auto set2 = [](u64* dst, u128h v) { dst[0] = (u64)v; dst[1] = (u64)(v >> 64); };
    set2(d.q_mod_t, q_mod_t); set2(d.t_half, t_half); set2(d.mask, mask); set2(d.neg_inv_q_mod_t, neg_inv_q); set2(d.inv_gamma_mod_t, inv_gamma);
    d.L = L; d.n = plan->n; d.t_bits = t_bits; d.elem_bytes = elem_bytes;
    *out = h.release();
    return TROYN_OK;
}

extern "C" uint64_t troyn_ring2k_gamma(const troyn_ring2k* h) { return h ? h->gamma : 0; }

static int ring2k_encode(const troyn_ring2k* h, bool scale, const void* src, size_t count, uint64_t* out, troyn_stream_t stream) {
    const char* P = scale ? "[PolynomialEncoderRNSHelper:scale_up]" : "[PolynomialEncoderRNSHelper:centralize]";
    if (!h || !out || (!src && count)) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (count > h->dev.n) return fail(TROYN_E_INVALID, std::string(P) + " source size is larger than poly_modulus_degree");
    const dim3 grid((h->dev.n + 255) / 256), block(256);
    if (scale) hipLaunchKernelGGL(ring2k_scale_up_kernel, grid, block, 0, (hipStream_t)stream, h->dev, src, (unsigned)count, (u64*)out);
    else hipLaunchKernelGGL(ring2k_centralize_kernel, grid, block, 0, (hipStream_t)stream, h->dev, src, (unsigned)count, (u64*)out);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_ring2k_scale_up(const troyn_ring2k* h, const void* src, size_t count, uint64_t* out, troyn_stream_t stream) {
    select_device(h); return ring2k_encode(h, true, src, count, out, stream); }
extern "C" int troyn_ring2k_centralize(const troyn_ring2k* h, const void* src, size_t count, uint64_t* out, troyn_stream_t stream) {
    select_device(h); return ring2k_encode(h, false, src, count, out, stream); }

extern "C" int troyn_ring2k_scale_down(const troyn_ring2k* h, const uint64_t* in, void* dst, troyn_stream_t stream) {
    select_device(h);
    if (!h || !in || !dst) return fail(TROYN_E_INVALID, "[PolynomialEncoderRNSHelper::scale_down] null argument");
    hipLaunchKernelGGL(ring2k_scale_down_kernel, dim3((h->dev.n + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->dev, (const u64*)in, dst);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_ring2k_decentralize(const troyn_ring2k* h, const uint64_t* in, void* dst, uint64_t correction_lo, uint64_t correction_hi, troyn_stream_t stream) {
    select_device(h);
    const char* P = "[PolynomialEncoderRNSHelper::decentralize]";
    if (!h || !in || !dst) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    typedef unsigned __int128 u128h;
    u128h cf = ((u128h)correction_hi << 64) | correction_lo;
    if (h->dev.elem_bytes == 4) cf &= 0xffffffffull; else if (h->dev.elem_bytes == 8) cf &= ~0ull;
    if ((cf & 1) == 0) return fail(TROYN_E_INVALID, "[bfv_ring2k::inverse_ring2k] x must be odd");
    u128h fix = cf;                                                  // Newton: the inverse modulo 2^128 (its low k bits are the inverse modulo 2^k)
    for (int it = 0; it < 8; it++) fix *= 2 - cf * fix;
    const u128h mask = h->dev.t_bits == 128 ? ~(u128h)0 : (((u128h)1 << h->dev.t_bits) - 1);
    fix &= mask;
    hipLaunchKernelGGL(ring2k_decentralize_kernel, dim3((h->dev.n + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->dev, (const u64*)in, dst, (u64)fix, (u64)(fix >> 64));
    LAUNCH_CHECK();
    return TROYN_OK;
}

// ---------------------------------------------------------------------------------------
// CKKS encoder (src/ckks_encoder.cu): canonical-embedding FFT, RNS reduction and CRT composition on the device
// ---------------------------------------------------------------------------------------
struct troyn_ckks {
    const troyn_plan* plan = nullptr;
    std::vector<uint32_t> index_map;                            // host copies (KAT hook)
    std::vector<std::complex<double>> roots, inv_roots;
    unsigned* d_slot_of = nullptr;                              // [N] inverse of index_map
    double2* d_roots = nullptr;                                 // [N]
    double2* d_inv_roots = nullptr;                             // [N]
    ulonglong2* d_garner = nullptr;                             // [K][K] q_j^-1 mod q_i, j < i
    u64* d_q_words = nullptr;                                   // [min(K, CKKS_MAX_L)][2][CKKS_MAX_L]: Q_L, floor(Q_L / 2)
    // ModRaise (raise_kernels.hpp)
    ulonglong2* d_radix = nullptr;                              // [K][CKKS_MAX_L] q_i mod q_j at [j][i]
    u64* d_half_digits = nullptr;                               // [CKKS_MAX_L][CKKS_MAX_L]: row L-1 = mixed-radix digits of floor(Q_L / 2)
    u64* d_q_mod = nullptr;                                     // [CKKS_MAX_L][K]: Q_L mod q_j at [L-1][j]
};

extern "C" int troyn_ckks_destroy(troyn_ckks* h) {
    if (!h) return TROYN_OK;
    for (void* p : {(void*)h->d_slot_of, (void*)h->d_roots, (void*)h->d_inv_roots, (void*)h->d_garner, (void*)h->d_q_words, (void*)h->d_radix, (void*)h->d_half_digits,
                    (void*)h->d_q_mod})
        if (p) (void)hipFree(p);
    delete h;
    return TROYN_OK;
}

extern "C" int troyn_ckks_create(troyn_ckks** out, const troyn_plan* plan) {
    const char* P = "[CKKSEncoder::CKKSEncoder]";
    if (!out || !plan) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    *out = nullptr;
    select_device(plan);
    std::unique_ptr<troyn_ckks, int (*)(troyn_ckks*)> h(new troyn_ckks, troyn_ckks_destroy);
    h->plan = plan;
    const size_t n = plan->n, K = plan->K;
    ckks_tables::build(plan->log_n, h->index_map, h->roots, h->inv_roots);
    std::vector<unsigned> slot_of(n);
    for (size_t i = 0; i < n; i++) slot_of[h->index_map[i]] = (unsigned)i;
    std::vector<double2> fwd(n), inv(n);
    for (size_t i = 0; i < n; i++) { fwd[i] = make_double2(h->roots[i].real(), h->roots[i].imag()); inv[i] = make_double2(h->inv_roots[i].real(), h->inv_roots[i].imag()); }
    std::vector<ulonglong2> garner(K * K, make_ulonglong2(0, 0));
    for (size_t i = 0; i < K; i++) for (size_t j = 0; j < i; j++) {
        const u64 qi = plan->moduli[i];
        u64 w = 0;
        if (!host::invmod(plan->moduli[j] % qi, qi, w)) return fail(TROYN_E_MODULUS, std::string(P) + " coeff_modulus is not pairwise coprime");
        garner[i * K + j] = shoup_pair(w, qi);
    }
    const size_t levels = std::min<size_t>(K, CKKS_MAX_L);
    std::vector<u64> words(levels * 2 * CKKS_MAX_L, 0);
    for (size_t L = 1; L <= levels; L++) {
        const std::vector<u64> big = host::big_product(std::vector<u64>(plan->moduli.begin(), plan->moduli.begin() + L));
        u64* qw = &words[(L - 1) * 2 * CKKS_MAX_L];
        for (size_t w = 0; w < big.size(); w++) qw[w] = big[w];
        for (size_t w = 0; w < (size_t)CKKS_MAX_L; w++) qw[CKKS_MAX_L + w] = (qw[w] >> 1) | (w + 1 < (size_t)CKKS_MAX_L ? qw[w + 1] << 63 : 0);
    }
    // ModRaise: q_i mod q_j for the Horner over the digits, and per input level L the mixed-radix digits of floor(Q_L / 2) and Q_L mod q_j
    std::vector<ulonglong2> radix(K * CKKS_MAX_L, make_ulonglong2(0, 0));
    for (size_t j = 0; j < K; j++) for (size_t i = 0; i < levels; i++) radix[j * CKKS_MAX_L + i] = shoup_pair(plan->moduli[i], plan->moduli[j]);
    std::vector<u64> half_digits((size_t)CKKS_MAX_L * CKKS_MAX_L, 0), q_mod((size_t)CKKS_MAX_L * K, 0);
    for (size_t L = 1; L <= levels; L++) {
        const u64* qw = &words[(L - 1) * 2 * CKKS_MAX_L];
        const std::vector<u64> big(qw, qw + CKKS_MAX_L);
        std::vector<u64> half(qw + CKKS_MAX_L, qw + 2 * CKKS_MAX_L);
        for (size_t i = 0; i < L; i++) half_digits[(L - 1) * CKKS_MAX_L + i] = host::big_divmod_small(half, plan->moduli[i]);
        for (size_t j = 0; j < K; j++) q_mod[(L - 1) * K + j] = host::big_mod_small(big, plan->moduli[j]);
    }
    if (int rc = upload_vector(&h->d_slot_of, slot_of)) return rc;
    if (int rc = upload_vector(&h->d_roots, fwd)) return rc;
    if (int rc = upload_vector(&h->d_inv_roots, inv)) return rc;
    if (int rc = upload_vector(&h->d_garner, garner)) return rc;
    if (int rc = upload_vector(&h->d_q_words, words)) return rc;
    if (int rc = upload_vector(&h->d_radix, radix)) return rc;
    if (int rc = upload_vector(&h->d_half_digits, half_digits)) return rc;
    if (int rc = upload_vector(&h->d_q_mod, q_mod)) return rc;
    *out = h.release();
    return TROYN_OK;
}

extern "C" int troyn_ckks_get_tables(const troyn_ckks* h, uint32_t* index_map, double* root_powers, double* inv_root_powers) {
    if (!h || !index_map || !root_powers || !inv_root_powers) return fail(TROYN_E_INVALID, "[troyn_ckks_get_tables] null argument");
    const size_t n = h->plan->n;
    for (size_t i = 0; i < n; i++) {
        index_map[i] = h->index_map[i];
        root_powers[2 * i] = h->roots[i].real(); root_powers[2 * i + 1] = h->roots[i].imag();
        inv_root_powers[2 * i] = h->inv_roots[i].real(); inv_root_powers[2 * i + 1] = h->inv_roots[i].imag();
    }
    return TROYN_OK;
}

namespace {
// the points between the two FFT passes come first (all an encoding needs: nothing at the one-pass sizes); decoding adds the residues of the inverse
// NTT and the real coefficients
struct CkksWorkspace { size_t work, residues, coeffs, total; };
inline size_t ckks_align(size_t b) { return (b + 255) & ~(size_t)255; }
CkksWorkspace ckks_workspace(const troyn_plan* p, size_t L, size_t batch, bool decode) {
    CkksWorkspace w;
    w.work = 0;
    w.residues = ckks_fft_two_pass(p->log_n) ? ckks_align(batch * p->n * sizeof(double2)) : 0;
    w.coeffs = w.residues + ckks_align(batch * L * p->n * sizeof(u64));
    w.total = decode ? w.coeffs + ckks_align(batch * p->n * sizeof(double)) : w.residues;
    return w;
}
}  // namespace

extern "C" size_t troyn_ckks_workspace_bytes(const troyn_ckks* h, uint32_t L, size_t batch) {
    if (!h || L < 1 || L > h->plan->K) return 0;
    return ckks_workspace(h->plan, L, batch, true).total;
}
extern "C" size_t troyn_ckks_encode_workspace_bytes(const troyn_ckks* h, size_t batch) {
    if (!h) return 0;
    return ckks_workspace(h->plan, 1, batch, false).total;
}

// what every entry checks the same way; 1: nothing to do (batch == 0)
static int ckks_check(const char* P, const troyn_ckks* h, uint32_t L, const void* in, const void* out, const void* ws, size_t ws_bytes, size_t batch, unsigned in_align, bool decode) {
    if (!h) return fail(TROYN_E_INVALID, std::string(P) + " null handle");
    if (L < 1 || L > h->plan->K) return fail(TROYN_E_INVALID, std::string(P) + " modulus count out of range");
    if (batch == 0) return 1;
    if (!in || !out) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (((uintptr_t)in & (in_align - 1)) || ((uintptr_t)out & 15) || ((uintptr_t)ws & 15)) return fail(TROYN_E_INVALID, std::string(P) + " misaligned pointer");
    if (batch << (h->plan->log_n - 8) > 0x7fffffffull || batch * L > 0x7fffffffull) return fail(TROYN_E_INVALID, std::string(P) + " batch too large for one launch");
    const size_t need = ckks_workspace(h->plan, L, batch, decode).total;
    if (ws_bytes < need || (need && !ws)) return fail(TROYN_E_WORKSPACE, std::string(P) + " workspace too small");
    return TROYN_OK;
}

// the source of troyn_ckks_encode_diagonals: `src` of ckks_encode is then the table, read through (diagonal, shift) pairs
struct CkksDiagonalSource { bool matrix; uint32_t n, nd; const uint32_t* pairs; };

static int ckks_encode(const troyn_ckks* h, bool simd, uint32_t L, const double* src, size_t count, double scale, uint64_t* out, uint32_t* too_large,
                       void* ws, size_t ws_bytes, size_t batch, troyn_stream_t stream, const CkksDiagonalSource* ds = nullptr) {
    const char* P = ds ? "[troyn_ckks_encode_diagonals]" : simd ? "[CKKSEncoder::encode_internal_complex_array]" : "[CKKSEncoder::encode_internal_double_polynomial]";
    select_device(h);
    // count == 0 reads nothing: a null source is then allowed
    alignas(16) static const double none[2] = {0, 0};
    const int rc = ckks_check(P, h, L, count ? (const void*)src : (const void*)none, out, ws, ws_bytes, batch, simd ? 16 : 8, false);
    if (rc < 0) return rc;
    if (rc == 1) return TROYN_OK;
    const troyn_plan* p = h->plan;
    if (count > (simd ? p->n / 2 : p->n)) return fail(TROYN_E_INVALID, std::string(P) + " Too many input values.");
    if (ds) {
        if (!ds->pairs) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
        if ((uintptr_t)ds->pairs & 3) return fail(TROYN_E_INVALID, std::string(P) + " misaligned pointer");
        if (ds->n == 0 || (ds->n & (ds->n - 1)) || ds->n > p->n / 2) return fail(TROYN_E_INVALID, std::string(P) + " n must be a power of two of at most N/2");
        if (!ds->matrix && ds->nd == 0) return fail(TROYN_E_INVALID, std::string(P) + " no diagonals");
    }
    size_t total_bits = 0;
    for (uint32_t i = 0; i < L; i++) total_bits += 64 - (size_t)__builtin_clzll(p->moduli[i]);
    if (!(scale > 0) || std::log2(scale) + 1.0 >= static_cast<double>(total_bits)) return fail(TROYN_E_INVALID, std::string(P) + " scale out of bounds.");
    if (too_large && ((uintptr_t)too_large & 3)) return fail(TROYN_E_INVALID, std::string(P) + " misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    if (too_large) HIP_TRY(hipMemsetAsync(too_large, 0, batch * sizeof(uint32_t), s));
    if (simd) {
        CkksFftArgs a;
        std::memset(&a, 0, sizeof(a));
        a.roots = h->d_inv_roots; a.slot_of = h->d_slot_of;
        a.values = reinterpret_cast<const double2*>(src); a.count = (unsigned)count;
        a.work = reinterpret_cast<double2*>((char*)ws + ckks_workspace(p, L, batch, false).work);
        a.residues = (u64*)out; a.mods = p->d_mods; a.L = L;
        a.fix = scale / static_cast<double>(p->n);
        a.too_large = too_large;
        if (ds) {
            a.values = nullptr;
            a.table = reinterpret_cast<const double2*>(src); a.pairs = reinterpret_cast<const uint2*>(ds->pairs);
            a.n_mask = ds->n - 1; a.n_log = (unsigned)__builtin_ctz(ds->n); a.a_max = ds->matrix ? ds->n - 1 : ds->nd - 1;
        }
        if (!(ds ? launch_ckks_fft_diagonals(p->log_n, ds->matrix, a, batch, s) : launch_ckks_fft(p->log_n, false, a, batch, s)))
            return fail(TROYN_E_UNSUPPORTED, std::string(P) + " no FFT kernel for this size");
    } else {
        launch_ckks_encode_polynomial(src, (unsigned)count, scale, p->n, p->d_mods, L, (u64*)out, too_large, batch, s);
    }
    LAUNCH_CHECK();
    NttArgs na = contiguous_args(p, (const u64*)out, (u64*)out, 1, L, 0, L, TROYN_IDX_COMPONENTWISE, 0);
    return launch_ntt(p, na, batch, false, s);
}

extern "C" int troyn_ckks_encode_simd(const troyn_ckks* h, uint32_t L, const double* values, size_t count, double scale, uint64_t* out, uint32_t* too_large,
                                      void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream) {
    return ckks_encode(h, true, L, values, count, scale, out, too_large, workspace, workspace_bytes, batch, stream);
}
extern "C" int troyn_ckks_encode_polynomial(const troyn_ckks* h, uint32_t L, const double* coeffs, size_t count, double scale, uint64_t* out, uint32_t* too_large,
                                            void* workspace, size_t workspace_bytes, size_t batch, troyn_stream_t stream) {
    return ckks_encode(h, false, L, coeffs, count, scale, out, too_large, workspace, workspace_bytes, batch, stream);
}

extern "C" size_t troyn_ckks_encode_diagonals_workspace_bytes(const troyn_ckks* h, size_t items) {
    return troyn_ckks_encode_workspace_bytes(h, items);
}
extern "C" int troyn_ckks_encode_diagonals(const troyn_ckks* h, uint32_t L, const double* src, int src_is_matrix, uint32_t n, uint32_t nd,
                                           const uint32_t* pairs, double scale, uint64_t* out, uint32_t* too_large,
                                           void* workspace, size_t workspace_bytes, size_t items, troyn_stream_t stream) {
    const CkksDiagonalSource ds = {src_is_matrix != 0, n, nd, pairs};
    return ckks_encode(h, true, L, src, h ? h->plan->n / 2 : 0, scale, out, too_large, workspace, workspace_bytes, items, stream, &ds);
}

// the number of present diagonals of the product of the layers [first, first + count) of the special DFT on n = N/2 slots; 0: nothing to write
static uint32_t ckks_dft_factor_count(const troyn_ckks* h, uint32_t first, uint32_t count) {
    if (!h || count == 0) return 0;
    const uint32_t m = h->plan->log_n - 1;
    if (first > m || count > m - first) return 0;
    return first + count == m ? 1u << count : (2u << count) - 1;
}

extern "C" size_t troyn_ckks_dft_factor_diagonals_count(const troyn_ckks* h, uint32_t first, uint32_t count) {
    return ckks_dft_factor_count(h, first, count);
}
extern "C" int troyn_ckks_dft_factor_diagonals(const troyn_ckks* h, uint32_t first, uint32_t count, int inverse, int col_mask, int row_mask, int conjugate,
                                               double constant, double* out, troyn_stream_t stream) {
    const char* P = "[troyn_ckks_dft_factor_diagonals]";
    if (!h) return fail(TROYN_E_INVALID, std::string(P) + " null handle");
    if (count == 0) return TROYN_OK;
    select_device(h);
    const uint32_t m = h->plan->log_n - 1;
    if (first > m || count > m - first) return fail(TROYN_E_INVALID, std::string(P) + " layers outside [0, log2 n]");
    if (col_mask < 0 || col_mask > 2 || row_mask < 0 || row_mask > 2) return fail(TROYN_E_INVALID, std::string(P) + " unknown mask");
    if (!std::isfinite(constant)) return fail(TROYN_E_INVALID, std::string(P) + " the constant is not finite");
    if (!out) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if ((uintptr_t)out & 15) return fail(TROYN_E_INVALID, std::string(P) + " misaligned pointer");
    CkksDftFactorArgs a{};
    a.roots = h->d_roots; a.out = reinterpret_cast<double2*>(out); a.constant = constant;
    a.log_n = h->plan->log_n; a.first = first; a.count = count;
    a.nd = ckks_dft_factor_count(h, first, count); a.wrap = first + count == m;
    a.inverse = inverse != 0; a.conjugate = conjugate != 0; a.col_mask = (unsigned)col_mask; a.row_mask = (unsigned)row_mask;
    launch_ckks_dft_factor(a, (hipStream_t)stream);
    LAUNCH_CHECK();
    return TROYN_OK;
}

// the same on the sub-ring of n slots: log2 n for a power of two 2 <= n <= N/2, 0 otherwise
static uint32_t ckks_sparse_log_slots(const troyn_ckks* h, uint32_t n) {
    if (!h || n < 2 || (n & (n - 1)) || n > (1u << (h->plan->log_n - 1))) return 0;
    uint32_t m = 0;
    while ((1u << m) < n) m++;
    return m;
}
static uint32_t ckks_dft_factor_sparse_count(const troyn_ckks* h, uint32_t n, uint32_t first, uint32_t count) {
    const uint32_t m = ckks_sparse_log_slots(h, n);
    if (m == 0 || count == 0) return 0;
    if (first > m || count > m - first) return 0;
    return first + count == m ? 1u << count : (2u << count) - 1;
}

extern "C" size_t troyn_ckks_dft_factor_diagonals_sparse_count(const troyn_ckks* h, uint32_t n, uint32_t first, uint32_t count) {
    return ckks_dft_factor_sparse_count(h, n, first, count);
}
extern "C" int troyn_ckks_dft_factor_diagonals_sparse(const troyn_ckks* h, uint32_t n, uint32_t first, uint32_t count, int inverse, int col_mask, int row_mask,
                                                      int conjugate, double constant, double* out, troyn_stream_t stream) {
    const char* P = "[troyn_ckks_dft_factor_diagonals_sparse]";
    if (!h) return fail(TROYN_E_INVALID, std::string(P) + " null handle");
    if (count == 0) return TROYN_OK;
    select_device(h);
    const uint32_t m = ckks_sparse_log_slots(h, n);
    if (m == 0) return fail(TROYN_E_INVALID, std::string(P) + " n must be a power of two in [2, N/2]");
    if (first > m || count > m - first) return fail(TROYN_E_INVALID, std::string(P) + " layers outside [0, log2 n]");
    if (col_mask < 0 || col_mask > 2 || row_mask < 0 || row_mask > 2) return fail(TROYN_E_INVALID, std::string(P) + " unknown mask");
    if (!std::isfinite(constant)) return fail(TROYN_E_INVALID, std::string(P) + " the constant is not finite");
    if (!out) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if ((uintptr_t)out & 15) return fail(TROYN_E_INVALID, std::string(P) + " misaligned pointer");
    CkksDftFactorSparseArgs a{};
    a.roots = h->d_roots; a.out = reinterpret_cast<double2*>(out); a.constant = constant;
    a.log_n = h->plan->log_n; a.log_slots = m; a.first = first; a.count = count;
    a.nd = ckks_dft_factor_sparse_count(h, n, first, count); a.wrap = first + count == m;
    a.inverse = inverse != 0; a.conjugate = conjugate != 0; a.col_mask = (unsigned)col_mask; a.row_mask = (unsigned)row_mask;
    launch_ckks_dft_factor_sparse(a, (hipStream_t)stream);
    LAUNCH_CHECK();
    return TROYN_OK;
}

// both halves on period 2n: log2 n for a power of two 2 <= n <= N/4, 0 otherwise
static uint32_t ckks_packed_log_slots(const troyn_ckks* h, uint32_t n) {
    if (!h || h->plan->log_n < 3 || n < 2 || (n & (n - 1)) || n > (1u << (h->plan->log_n - 2))) return 0;
    uint32_t m = 0;
    while ((1u << m) < n) m++;
    return m;
}
static uint32_t ckks_dft_factor_packed_count(const troyn_ckks* h, uint32_t n, uint32_t first, uint32_t count) {
    const uint32_t m = ckks_packed_log_slots(h, n);
    if (m == 0 || count == 0) return 0;
    if (first > m || count > m - first) return 0;
    return (2u << count) - 1;
}

extern "C" size_t troyn_ckks_dft_factor_diagonals_packed_count(const troyn_ckks* h, uint32_t n, uint32_t first, uint32_t count) {
    return ckks_dft_factor_packed_count(h, n, first, count);
}
extern "C" int troyn_ckks_dft_factor_diagonals_packed(const troyn_ckks* h, uint32_t n, uint32_t first, uint32_t count, int inverse, double constant, double* out,
                                                      troyn_stream_t stream) {
    const char* P = "[troyn_ckks_dft_factor_diagonals_packed]";
    if (!h) return fail(TROYN_E_INVALID, std::string(P) + " null handle");
    if (count == 0) return TROYN_OK;
    select_device(h);
    const uint32_t m = ckks_packed_log_slots(h, n);
    if (m == 0) return fail(TROYN_E_INVALID, std::string(P) + " n must be a power of two in [2, N/4]");
    if (first > m || count > m - first) return fail(TROYN_E_INVALID, std::string(P) + " layers outside [0, log2 n]");
    if (!std::isfinite(constant)) return fail(TROYN_E_INVALID, std::string(P) + " the constant is not finite");
    if (!out) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if ((uintptr_t)out & 15) return fail(TROYN_E_INVALID, std::string(P) + " misaligned pointer");
    CkksDftFactorPackedArgs a{};
    a.roots = h->d_roots; a.out = reinterpret_cast<double2*>(out); a.constant = constant;
    a.log_n = h->plan->log_n; a.log_rows = m + 1; a.first = first; a.count = count;
    a.nd = ckks_dft_factor_packed_count(h, n, first, count);
    a.inverse = inverse != 0;
    launch_ckks_dft_factor_packed(a, (hipStream_t)stream);
    LAUNCH_CHECK();
    return TROYN_OK;
}

static int ckks_decode(const troyn_ckks* h, bool simd, uint32_t L, const uint64_t* plain, double scale, double* out, void* ws, size_t ws_bytes, size_t batch,
                       troyn_stream_t stream) {
    const char* P = "[CKKSEncoder::decode_internal]";
    select_device(h);
    const int rc = ckks_check(P, h, L, plain, out, ws, ws_bytes, batch, 16, true);
    if (rc < 0) return rc;
    if (rc == 1) return TROYN_OK;
    if (L > (uint32_t)CKKS_MAX_L) return fail(TROYN_E_UNSUPPORTED, std::string(P) + " more than 16 moduli");
    const troyn_plan* p = h->plan;
    hipStream_t s = (hipStream_t)stream;
    const CkksWorkspace w = ckks_workspace(p, L, batch, true);
    u64* residues = reinterpret_cast<u64*>((char*)ws + w.residues);
    double* coeffs = simd ? reinterpret_cast<double*>((char*)ws + w.coeffs) : out;
    NttArgs na = contiguous_args(p, (const u64*)plain, residues, 1, L, 0, L, TROYN_IDX_COMPONENTWISE, 0);
    if (int r = launch_ntt(p, na, batch, true, s)) return r;
    CkksComposeArgs c;
    std::memset(&c, 0, sizeof(c));
    c.residues = residues; c.mods = p->d_mods; c.garner = h->d_garner; c.K = p->K; c.L = L; c.n = p->n;
    c.q_words = h->d_q_words + (size_t)(L - 1) * 2 * CKKS_MAX_L; c.half_words = c.q_words + CKKS_MAX_L;
    c.scale = scale; c.out = coeffs;
    if (!launch_ckks_compose(c, batch, s)) return fail(TROYN_E_UNSUPPORTED, std::string(P) + " more than 16 moduli");
    if (simd) {
        CkksFftArgs a;
        std::memset(&a, 0, sizeof(a));
        a.roots = h->d_roots; a.slot_of = h->d_slot_of; a.coeffs = coeffs;
        a.work = reinterpret_cast<double2*>((char*)ws + w.work);
        a.slots = reinterpret_cast<double2*>(out);
        if (!launch_ckks_fft(p->log_n, true, a, batch, s)) return fail(TROYN_E_UNSUPPORTED, std::string(P) + " no FFT kernel for this size");
    }
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_ckks_decode_polynomial(const troyn_ckks* h, uint32_t L, const uint64_t* plain, double scale, double* out, void* workspace, size_t workspace_bytes,
                                            size_t batch, troyn_stream_t stream) {
    return ckks_decode(h, false, L, plain, scale, out, workspace, workspace_bytes, batch, stream);
}
extern "C" int troyn_ckks_decode_simd(const troyn_ckks* h, uint32_t L, const uint64_t* plain, double scale, double* out, void* workspace, size_t workspace_bytes,
                                      size_t batch, troyn_stream_t stream) {
    return ckks_decode(h, true, L, plain, scale, out, workspace, workspace_bytes, batch, stream);
}

// ---- ModRaise: the centred base extension of [batch][pcount][L_in][N] to [batch][pcount][L_out][N] (raise_kernels.hpp) ----
namespace {
// NTT form: the inverse transforms of the input rows, then the new rows in coefficient form; coefficient form: nothing
struct RaiseWorkspace { size_t coeffs, fresh, total; };
RaiseWorkspace raise_workspace(const troyn_plan* p, size_t L_in, size_t L_out, size_t pcount, size_t batch, bool ntt) {
    RaiseWorkspace w;
    w.coeffs = 0;
    w.fresh = ntt ? ckks_align(batch * pcount * L_in * p->n * sizeof(u64)) : 0;
    w.total = ntt ? w.fresh + ckks_align(batch * pcount * (L_out - L_in) * p->n * sizeof(u64)) : 0;
    return w;
}
inline bool raise_levels_ok(const troyn_ckks* h, uint32_t L_in, uint32_t L_out) { return L_in >= 1 && L_in < L_out && L_out <= h->plan->K; }
}  // namespace

extern "C" size_t troyn_ckks_mod_raise_workspace_bytes(const troyn_ckks* h, uint32_t L_in, uint32_t L_out, size_t pcount, size_t batch, int is_ntt_form) {
    if (!h || !raise_levels_ok(h, L_in, L_out)) return 0;
    return raise_workspace(h->plan, L_in, L_out, pcount, batch, is_ntt_form != 0).total;
}

extern "C" int troyn_ckks_mod_raise(const troyn_ckks* h, uint32_t L_in, uint32_t L_out, int is_ntt_form, const uint64_t* in, size_t pcount,
                                    uint64_t* out, void* ws, size_t ws_bytes, size_t batch, troyn_stream_t stream) {
    const std::string P = "[troyn_ckks_mod_raise]";
    select_device(h);
    if (!h) return fail(TROYN_E_INVALID, P + " null handle");
    if (!raise_levels_ok(h, L_in, L_out)) return fail(TROYN_E_INVALID, P + " limb counts out of range (1 <= L_in < L_out <= n_moduli)");
    const size_t items = batch * pcount;
    if (items == 0) return TROYN_OK;
    if (!in || !out) return fail(TROYN_E_INVALID, P + " null argument");
    if (((uintptr_t)in & 15) || ((uintptr_t)out & 15) || ((uintptr_t)ws & 15)) return fail(TROYN_E_INVALID, P + " misaligned pointer");
    const troyn_plan* p = h->plan;
    const size_t n = p->n;
    {
        const uintptr_t i0 = (uintptr_t)in, i1 = i0 + items * L_in * n * sizeof(u64), o0 = (uintptr_t)out, o1 = o0 + items * L_out * n * sizeof(u64);
        if (i0 < o1 && o0 < i1) return fail(TROYN_E_INVALID, P + " `out` overlaps `in`");
    }
    const unsigned ch = chunks_pairs(p->n);
    if (int rc = check_rows(items * L_out, ch)) return rc;
    const bool ntt = is_ntt_form != 0;
    const RaiseWorkspace w = raise_workspace(p, L_in, L_out, pcount, batch, ntt);
    if (ws_bytes < w.total || (w.total && !ws)) return fail(TROYN_E_WORKSPACE, P + " workspace too small");
    if (L_in > (uint32_t)CKKS_MAX_L) return fail(TROYN_E_UNSUPPORTED, P + " more than 16 input moduli");
    hipStream_t s = (hipStream_t)stream;
    const unsigned fresh_rows = L_out - L_in;
    ModRaiseArgs a;
    std::memset(&a, 0, sizeof(a));
    a.mods = p->d_mods; a.garner = h->d_garner; a.radix = h->d_radix;
    a.half_digits = h->d_half_digits + (size_t)(L_in - 1) * CKKS_MAX_L; a.q_mod = h->d_q_mod + (size_t)(L_in - 1) * p->K;
    a.K = p->K; a.L = L_in; a.LO = L_out; a.n = p->n;
    if (!ntt) {
        // the kernel writes all L_out rows: the low rows as it read them
        a.in = (const u64*)in; a.low = (u64*)out; a.low_stride = (size_t)L_out * n;
        a.out = (u64*)out + (size_t)L_in * n; a.out_stride = (size_t)L_out * n;
        if (!launch_ckks_mod_raise(a, items, ch, s)) return fail(TROYN_E_UNSUPPORTED, P + " more than 16 input moduli");
        LAUNCH_CHECK();
        return TROYN_OK;
    }
    // NTT o extend o INTT: the low rows are copied, the L_in input rows take the inverse transform, the new rows the forward one
    u64* coeffs = reinterpret_cast<u64*>((char*)ws + w.coeffs);
    u64* fresh = reinterpret_cast<u64*>((char*)ws + w.fresh);
    hipLaunchKernelGGL(copy_limbs_kernel, dim3((unsigned)(items * L_in * ch)), dim3(POLY_BLOCK), 0, s,
                       ch, p->n, (const u64*)in, (size_t)L_in * n, 0u, (u64*)out, (size_t)L_out * n, L_in);
    LAUNCH_CHECK();
    NttArgs ia = contiguous_args(p, (const u64*)in, coeffs, pcount, L_in, 0, L_in, TROYN_IDX_COMPONENTWISE, 0);
    if (int rc = launch_ntt(p, ia, batch, true, s)) return rc;
    a.in = coeffs; a.low = nullptr; a.out = fresh; a.out_stride = (size_t)fresh_rows * n;
    if (!launch_ckks_mod_raise(a, items, ch, s)) return fail(TROYN_E_UNSUPPORTED, P + " more than 16 input moduli");
    LAUNCH_CHECK();
    NttArgs fa = contiguous_args(p, fresh, (u64*)out + (size_t)L_in * n, pcount, fresh_rows, L_in, fresh_rows, TROYN_IDX_COMPONENTWISE, 0);
    fa.out_pstride = (long long)L_out * n; fa.out_bstride = (long long)pcount * L_out * n;
    return launch_ntt(p, fa, batch, false, s);
}

extern "C" size_t troyn_gather_workspace_bytes(size_t count) { return (count + 1) * sizeof(u64); }

extern "C" int troyn_gather(const uint64_t* const* src, size_t count, size_t words, uint64_t* out, void* workspace, size_t workspace_bytes, troyn_stream_t stream) {
    if (!src || !out || !workspace) return fail(TROYN_E_INVALID, "[troyn_gather] null argument");
    if (count == 0 || words == 0) return TROYN_OK;
    if (count > 65535) return fail(TROYN_E_INVALID, "[troyn_gather] batch too large for one launch");
    if (workspace_bytes < troyn_gather_workspace_bytes(count)) return fail(TROYN_E_WORKSPACE, "[troyn_gather] workspace too small");
    for (size_t i = 0; i < count; i++)
        if (!src[i] || ((uintptr_t)src[i] & 15)) return fail(TROYN_E_INVALID, "[troyn_gather] null or misaligned pointer in the batch");
    if ((uintptr_t)out & 15) return fail(TROYN_E_INVALID, "[troyn_gather] misaligned destination");
    hipStream_t s = (hipStream_t)stream;
    const unsigned bx = (unsigned)std::min<size_t>((words / 2 + 255) / 256 + 1, 64);
    if (count <= 64) {   // pointers by value: no upload, no host wait
        GatherPtrs g;
        for (size_t i = 0; i < 64; i++) g.p[i] = reinterpret_cast<const u64*>(src[i < count ? i : 0]);
        hipLaunchKernelGGL(gather_small_kernel, dim3(bx, (unsigned)count), dim3(256), 0, s, g, words, (u64*)out);
        LAUNCH_CHECK();
        return TROYN_OK;
    }
    if (int rc = upload_host_table(s, workspace, src, count * sizeof(u64))) return rc;
    hipLaunchKernelGGL(gather_kernel, dim3(bx, (unsigned)count), dim3(256), 0, s, (const u64* const*)workspace, words, (u64*)out);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" int troyn_scatter(const uint64_t* in, uint64_t* const* dst, size_t count, size_t words, void* workspace, size_t workspace_bytes, troyn_stream_t stream) {
    if (!in || !dst || !workspace) return fail(TROYN_E_INVALID, "[troyn_scatter] null argument");
    if (count == 0 || words == 0) return TROYN_OK;
    if (count > 65535) return fail(TROYN_E_INVALID, "[troyn_scatter] batch too large for one launch");
    if (workspace_bytes < troyn_gather_workspace_bytes(count)) return fail(TROYN_E_WORKSPACE, "[troyn_scatter] workspace too small");
    for (size_t i = 0; i < count; i++)
        if (!dst[i] || ((uintptr_t)dst[i] & 15)) return fail(TROYN_E_INVALID, "[troyn_scatter] null or misaligned pointer in the batch");
    if ((uintptr_t)in & 15) return fail(TROYN_E_INVALID, "[troyn_scatter] misaligned source");
    hipStream_t s = (hipStream_t)stream;
    const unsigned bx = (unsigned)std::min<size_t>((words / 2 + 255) / 256 + 1, 64);
    if (count <= 64) {
        ScatterPtrs g;
        for (size_t i = 0; i < 64; i++) g.p[i] = reinterpret_cast<u64*>(dst[i < count ? i : 0]);
        hipLaunchKernelGGL(scatter_small_kernel, dim3(bx, (unsigned)count), dim3(256), 0, s, (const u64*)in, g, words);
        LAUNCH_CHECK();
        return TROYN_OK;
    }
    if (int rc = upload_host_table(s, workspace, dst, count * sizeof(u64))) return rc;
    hipLaunchKernelGGL(scatter_kernel, dim3(bx, (unsigned)count), dim3(256), 0, s, (const u64*)in, (u64* const*)workspace, words);
    LAUNCH_CHECK();
    return TROYN_OK;
}

extern "C" size_t troyn_multiply_plain_accumulate_workspace_bytes(size_t count) { return (4 * count + 2) * sizeof(u64); }

extern "C" int troyn_multiply_plain_accumulate(const troyn_plan* p, uint32_t mod_start, uint32_t nmod, size_t pcount,
                                               const uint64_t* const* ct, const uint64_t* const* pt, uint64_t* const* dst, size_t count,
                                               int set_zero, void* workspace, size_t workspace_bytes, troyn_stream_t stream) {
    select_device(p);
    const char* P = "[Evaluator::multiply_plain_ntt_batched]";
    if (!p || !ct || !pt || !dst || !workspace) return fail(TROYN_E_INVALID, std::string(P) + " null argument");
    if (nmod == 0 || mod_start + nmod > p->K) return fail(TROYN_E_INVALID, std::string(P) + " modulus slice out of range");
    if (count == 0 || pcount == 0) return TROYN_OK;
    if (workspace_bytes < troyn_multiply_plain_accumulate_workspace_bytes(count)) return fail(TROYN_E_WORKSPACE, "[troyn_multiply_plain_accumulate] workspace too small");
    if (count > 0x7fffffffull) return fail(TROYN_E_INVALID, std::string(P) + " too many terms");
    // group the terms by destination (stable), so that each destination is produced by one pass over its terms
    std::vector<size_t> order(count);
    for (size_t i = 0; i < count; i++) {
        if (!ct[i] || !pt[i] || !dst[i]) return fail(TROYN_E_INVALID, std::string(P) + " null pointer in the batch");
        order[i] = i;
    }
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return (uintptr_t)dst[a] < (uintptr_t)dst[b]; });
    std::vector<u64> tab(2 * count);
    std::vector<u64> gdst, gstart;
    for (size_t i = 0; i < count; i++) {
        const size_t k = order[i];
        tab[i] = (u64)(uintptr_t)ct[k];
        tab[count + i] = (u64)(uintptr_t)pt[k];
        if (i == 0 || dst[k] != dst[order[i - 1]]) { gdst.push_back((u64)(uintptr_t)dst[k]); gstart.push_back((u64)i); }
    }
    gstart.push_back((u64)count);
    const size_t groups = gdst.size();
    tab.insert(tab.end(), gdst.begin(), gdst.end());
    tab.insert(tab.end(), gstart.begin(), gstart.end());
    hipStream_t s = (hipStream_t)stream;
    if (int rc = upload_host_table(s, workspace, tab.data(), tab.size() * sizeof(u64))) return rc;
    const unsigned ch = chunks_pairs(p->n);
    const int pm = p->opt.plain_mac;          // TROYN_PLAIN_MAC: 1 v1 (the kernel of pcount != 2, one polynomial per thread), 2 single, 3 dual, 4 quad
    const int mac_gen = pm == 1 ? 1 : 2;
    if (pcount == 2 && mac_gen == 2) {
        const size_t rows2 = groups * nmod;
        if (int rc = check_rows(rows2, ch)) return rc;
        TimerScope ts(TROYN_TIMER_PLAIN_MAC, s);
        // ND consecutive destinations with the same ciphertext operands term by term (the columns of a matmul row) share one workgroup: every
        // ciphertext word is loaded once for all of them (TROYN_PLAIN_MAC=single / dual / quad forces the grouping; A/B, tests)
        auto shared_operands = [&](size_t nd) {
            if (groups < nd || groups % nd != 0) return false;
            for (size_t g = 0; g < groups; g += nd) {
                const size_t a0 = (size_t)gstart[g], len = (size_t)gstart[g + 1] - a0;
                for (size_t d = 1; d < nd; d++) {
                    const size_t b0 = (size_t)gstart[g + d];
                    if ((size_t)gstart[g + d + 1] - b0 != len || b0 != a0 + d * len) return false;
                    for (size_t j = 0; j < len; j++) if (tab[a0 + j] != tab[b0 + j]) return false;
                }
            }
            return true;
        };
        size_t nd = 1;
        if (pm != 2) {
            if (pm != 3 && shared_operands(4)) nd = 4;
            else if (pm != 4 && shared_operands(2)) nd = 2;
        }
        if (nd > 1) {
            const size_t rowsd = (groups / nd) * nmod;
            if (nd == 4)
                hipLaunchKernelGGL((plain_mac2_multi_kernel<2, 4>), dim3((unsigned)(rowsd * ch)), dim3(POLY_BLOCK), 0, s,
                                   ch, p->d_mods, mod_start, nmod, p->n, (const u64*)workspace, (unsigned)count, (unsigned)groups, set_zero ? 1 : 0);
            else
                hipLaunchKernelGGL((plain_mac2_multi_kernel<2, 2>), dim3((unsigned)(rowsd * ch)), dim3(POLY_BLOCK), 0, s,
                                   ch, p->d_mods, mod_start, nmod, p->n, (const u64*)workspace, (unsigned)count, (unsigned)groups, set_zero ? 1 : 0);
            LAUNCH_CHECK();
            return TROYN_OK;
        }
        // (the packed weight layout of round 4 -- plain_mac2_kernel<2, true>, 0.506 -> 0.537 of HBM, profiles/r04_plain_mac_ab.txt -- was a
        // development experiment with a second plaintext representation; its instantiation left the library in round 5)
        hipLaunchKernelGGL((plain_mac2_kernel<2>), dim3((unsigned)(rows2 * ch)), dim3(POLY_BLOCK), 0, s,
                           ch, p->d_mods, mod_start, nmod, p->n, (const u64*)workspace, (unsigned)count, (unsigned)groups, set_zero ? 1 : 0);
        LAUNCH_CHECK();
        return TROYN_OK;
    }
    const size_t rows = groups * pcount * nmod;
    if (int rc = check_rows(rows, ch)) return rc;
    hipLaunchKernelGGL(plain_mac_kernel, dim3((unsigned)(rows * ch)), dim3(POLY_BLOCK), 0, s,
                       ch, p->d_mods, mod_start, nmod, p->n, (unsigned)pcount, (const u64*)workspace, (unsigned)count, (unsigned)groups, set_zero ? 1 : 0);
    LAUNCH_CHECK();
    return TROYN_OK;
}
