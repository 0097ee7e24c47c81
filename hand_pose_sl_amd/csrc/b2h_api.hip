// libb2h.so -- C ABI (include/b2h.h) over the gfx950 kernels.
// Host side: argument checks mirroring the reference's errors, weight repacking
// into the kernels' fragment layouts, launches on the caller's stream.
#include "../../include/b2h.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "b2h_common.h"
#include "kernel_mfma.h"
#include "kernel_mfma16.h"
#include "kernel_mfma16w.h"
#include "kernel_mfma3.h"
#include "kernel_mfma3w.h"
#include "kernel_tenc.h"
#include "kernel_tenc_train.h"
#include "kernel_train_attn.h"
#include "kernel_tpt.h"
#include "kernel_attn_long.h"
#include "kernel_adam.h"
#include "kernel_step_control.h"
#include "kernel_build_batch.h"
#include "kernel_build_batch_aug.h"
#include "kernel_scatter_rows.h"
#include "kernel_dropout_masks.h"
#include "kernel_epoch_plan.h"
#include "kernel_token_lengths.h"
#include "kernel_train_attn_long.h"
#include "kernel_train_attn_mfma.h"
#include "kernel_train_linear_mfma.h"
#include "kernel_train_attn_whole_mfma.h"
#include "kernel_tpt_train.h"
#include "kernel_train.h"
#include "kernel_valu.h"

using namespace b2h;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return fail(B2H_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

uint16_t f32_to_bf16(float f) { // round-to-nearest-even
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)((u >> 16) | ((u & 0xffffu) ? 0x40u : 0u));
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

uint16_t f32_to_f16(float f) { // round-to-nearest-even, IEEE binary16
    uint32_t u;
    std::memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const uint32_t absu = u & 0x7fffffffu;
    if (absu >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | ((absu > 0x7f800000u) ? 0x200u : 0u));
    if (absu >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u); // rounds to >= 65520 -> inf
    if (absu < 0x38800000u) { // below 2^-14: subnormal half, grid 2^-24
        float a;
        std::memcpy(&a, &absu, 4);
        const uint32_t m = (uint32_t)std::nearbyintf(a * 16777216.0f);
        return (uint16_t)(sign | m);
    }
    uint32_t r = absu + 0xfffu + ((absu >> 13) & 1u);
    return (uint16_t)(sign | ((r - 0x38000000u) >> 13));
}

// hipEvent_t that is destroyed on every exit path
struct Event {
    hipEvent_t e = nullptr;
    ~Event() { if (e) (void)hipEventDestroy(e); }
};

// The library binds a model to the device current at creation; a launch from another current
// device would run a kernel there that dereferences this device's weights.
int check_device(int model_device) {
    int cur = -1;
    HIP_TRY(hipGetDevice(&cur));
    if (cur != model_device)
        return fail(B2H_ERR_INVALID, "model is bound to HIP device " + std::to_string(model_device) +
                                        ", the current device is " + std::to_string(cur));
    return B2H_OK;
}

// The model-free entry points (metric, target transform) have no device of their own: every pointer
// must be non-NULL device memory of the CURRENT device, or the kernel would fault / run elsewhere.
int check_device_ptr(const void* p, const char* name) {
    if (!p) return fail(B2H_ERR_INVALID, std::string(name) + " is NULL");
    int cur = -1;
    HIP_TRY(hipGetDevice(&cur));
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(B2H_ERR_INVALID, std::string(name) + " is not a device pointer");
    }
    if (a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged)
        return fail(B2H_ERR_INVALID, std::string(name) + " is not device memory");
    if (a.device != cur)
        return fail(B2H_ERR_INVALID, std::string(name) + " lives on HIP device " + std::to_string(a.device) +
                                        ", the current device is " + std::to_string(cur));
    return B2H_OK;
}

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int upload(const void* host, size_t n) {
        if (p && bytes != n) { (void)hipFree(p); p = nullptr; }
        if (!p) HIP_TRY(hipMalloc(&p, n));
        bytes = n;
        HIP_TRY(hipMemcpy(p, host, n, hipMemcpyHostToDevice));
        return B2H_OK;
    }
};

bool overlaps(const void* a, size_t an, const void* b, size_t bn) {
    const char* x = reinterpret_cast<const char*>(a);
    const char* y = reinterpret_cast<const char*>(b);
    return x < y + bn && y < x + an;
}

bool misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) & (a - 1); }

// An operand of a training entry point: n bytes at p.  `what` names a read-only one in check_overlap's message.
struct Span {
    const void* p;
    size_t n;
    const char* what = nullptr;
};

// No output may overlap a read-only operand (an input, a parameter, a mask) or another output.
int check_overlap(const std::vector<Span>& outs, const std::vector<Span>& read_only) {
    for (size_t a = 0; a < outs.size(); ++a) {
        for (const Span& r : read_only)
            if (overlaps(outs[a].p, outs[a].n, r.p, r.n)) return fail(B2H_ERR_INVALID, std::string("an output overlaps ") + r.what);
        for (size_t c = a + 1; c < outs.size(); ++c)
            if (overlaps(outs[a].p, outs[a].n, outs[c].p, outs[c].n)) return fail(B2H_ERR_INVALID, "two outputs overlap");
    }
    return B2H_OK;
}

// An operand of a data-path entry point (build_batch, scatter_rows, b2h_epoch_plan, b2h_joint_error): what a message
// calls it, where it lies, its bytes, the alignment the call promises, whether the call may leave it out, whether it is
// written.  A table of them is checked in its own order, so the read-only operands stand before the outputs.
struct Op {
    const char* name;
    const void* p;
    size_t n;
    uintptr_t align;
    bool optional, out;
};

// Operand by operand: a missing one that is not optional, then a misaligned one.
int check_ops_given(const Op* ops, size_t count) {
    for (const Op* o = ops; o < ops + count; ++o) {
        if (!o->p && !o->optional) return fail(B2H_ERR_INVALID, std::string(o->name) + " is NULL");
        if (misaligned(o->p, o->align))
            return fail(B2H_ERR_INVALID, std::string(o->name) + " must be " + std::to_string(o->align) + "-byte aligned");
    }
    return B2H_OK;
}

// check_overlap over the operands that are given, then check_device_ptr on those that have bytes.  An operand of zero
// bytes takes part in the overlap check only with `empty_overlaps` (it then collides with a span it lies strictly
// inside): the entry points differ in this and callers can see it.
int check_ops_memory(const Op* ops, size_t count, bool empty_overlaps) {
    std::vector<Span> out_spans, in_spans;
    for (const Op* o = ops; o < ops + count; ++o)
        if (o->p && (o->n || empty_overlaps)) (o->out ? out_spans : in_spans).push_back({o->p, o->n, o->name});
    if (int rc = check_overlap(out_spans, in_spans)) return rc;
    for (const Op* o = ops; o < ops + count; ++o)
        if (o->p && o->n)
            if (int rc = check_device_ptr(o->p, o->name)) return rc;
    return B2H_OK;
}

template <size_t N> int check_ops(const Op (&ops)[N], bool empty_overlaps) {
    if (int rc = check_ops_given(ops, N)) return rc;
    return check_ops_memory(ops, N, empty_overlaps);
}

// Host copies of a model's fp32 tensors (non-NULL; host memory, or memory of the current device) of the given
// sizes in floats.  Returns after the device is idle: no launch may still read the old packed buffers.
int fetch_tensors(const float* const* tensors, const std::vector<size_t>& sizes, int on_device,
                  std::vector<std::vector<float>>& out) {
    out.resize(sizes.size());
    for (size_t i = 0; i < sizes.size(); ++i) {
        out[i].resize(sizes[i]);
        if (on_device) HIP_TRY(hipMemcpy(out[i].data(), tensors[i], sizes[i] * 4, hipMemcpyDeviceToHost));
        else std::memcpy(out[i].data(), tensors[i], sizes[i] * 4);
    }
    HIP_TRY(hipDeviceSynchronize());
    return B2H_OK;
}

// The current HIP device, which a new model is bound to: it must be a gfx950.
int probe_device(int& device, int& num_cus) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return fail(B2H_ERR_NO_DEVICE, "no HIP device visible (libb2h has no CPU path)");
    HIP_TRY(hipGetDevice(&device));
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, device));
    if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
        return fail(B2H_ERR_NO_DEVICE, std::string("device is ") + p.gcnArchName + ", libb2h is built for gfx950 only");
    num_cus = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
    return B2H_OK;
}

// Flags and factor of the *_forward_fused entry points.
int check_fused(int flags, float factor) {
    if (flags & ~(kPreChest | kPreNorm | kPostDenorm | kPostMask)) return fail(B2H_ERR_INVALID, "unknown flag bits");
    if ((flags & (kPreNorm | kPostDenorm)) && !(factor > 0.f)) return fail(B2H_ERR_INVALID, "factor must be > 0");
    return B2H_OK;
}

// Every kernel that may use more than 64 KB of dynamic LDS gets its cap raised ONCE per device (OncePerDevice),
// when a model is created or its weights are loaded -- not inside a launch, so that the very first forward is
// already free of runtime calls other than the launches themselves and can be captured into a HIP graph.
template <typename K> int raise_lds_cap(K kern, int bytes = 160 * 1024) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return B2H_OK;
}

// Runs a setter of kernel attributes (which are per device) once for each device.
struct OncePerDevice {
    std::mutex mu;
    bool done[64] = {};
    template <typename F> int operator()(F set) {
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lock(mu);
        if (dev >= 0 && dev < 64 && done[dev]) return B2H_OK;
        if (int rc = set()) return rc;
        if (dev >= 0 && dev < 64) done[dev] = true;
        return B2H_OK;
    }
};

// Element kinds of the matrix-core weight fragments; also the index of b2h_model::pk.
enum Elem { EL_BF16, EL_F16, EL_F16X3, EL_F32, kElems };

// The packed weights of one wave-per-chunk kernel variant: per-layer fragments (the bias is b2h_model::bias).
struct Packed {
    DevBuf w[4];
    MfmaParams mp{};
};

} // namespace

constexpr int kPoolSlots = 64;        // streams per model that get a chunk pool (Sched16); further streams run without
constexpr int kPoolSlotBytes = 128;   // one cache line per slot
constexpr int64_t kPoolMinChunks = 256; // chunks per workgroup from which a launch is dynamic (at 64 it measured 2.5 % slower than static)

struct b2h_model {
    int C = 0;
    int pos_emb = 0;
    int device = 0;
    bool has_weights = false;
    int cin[4], cout[4];
    // packed device weights
    DevBuf valu_w[4], valu_b[4];
    Packed pk[kElems]; // wave-per-chunk matrix-core kernels by element kind (<= 32 channels: F16X3 and F32 only)
    DevBuf bias[4];    // their bias fragments, one per layer: the out-slot order is the same for every element kind
    DevBuf img16[2];   // persistent 16-bit kernel, bf16 / f16: [W L0..L3 | bias L0..L3], kPacked16 bytes
    int num_cus = 256;
    // Chunk pools of the persistent 16-bit kernel (kernel_mfma16.h, Sched16): one 128-byte slot per stream
    // that has launched on this model, two words each (claim counter, finished workgroups), zero between
    // launches.  Launches on one stream are ordered, so a slot is never shared by two running kernels -- as long
    // as one handle value names one ordered queue: hipStreamPerThread does not and never gets a slot (pool_slot()).
    DevBuf pools;
    std::mutex pool_mu;
    std::vector<hipStream_t> pool_streams;
    ValuParams vp;
    float w_absmax = 0.f;         // largest |weight| or |bias| (NaN counts as inf): F16X3 needs < 65504
};

namespace {

int round_up(int v, int m) { return (v + m - 1) / m * m; }

// value of weight (layer l, out-channel o, in-channel slot i, tap k); in-channel
// slot order of layer 1 with pos_emb: slots 0..23 = reference channels 1..24
// (keypoints), slot 24 = reference channel 0 (t/100).
struct HostWeights {
    const b2h_model* m;
    std::vector<float> w[4], b[4];
    float at(int l, int o, int slot, int k, bool permute_pos) const {
        if (o >= m->cout[l] || slot >= m->cin[l]) return 0.f;
        int i = slot;
        if (l == 0 && m->pos_emb && permute_pos) i = (slot == 24) ? 0 : slot + 1;
        return w[l][((size_t)o * m->cin[l] + i) * kTaps + k];
    }
    float bias(int l, int o) const { return o < m->cout[l] ? b[l][o] : 0.f; }
};

constexpr float kF16Max = 65504.f;

// largest magnitude of a set of fp32 values; a NaN makes it +inf
float absmax_of(const std::vector<float>& v, float acc) {
    for (float x : v) {
        const float a = std::fabs(x);
        if (!(a <= acc)) acc = std::isnan(a) ? INFINITY : a;
    }
    return acc;
}

// Fragment geometry of layer l in the narrow (<= 32 channels) or wide (33..64) matrix-core kernels: M-tiles,
// k-steps of 4E inputs (16-bit: k-steps of 32, fp32: k-groups of 16) and out slot (mt, row) -> channel.
struct FragGeo {
    int mt, ks;
    int (*chan)(int mt, int row);
};

FragGeo frag_geo(bool wide, int l, bool f32) {
    int (*chan)(int, int) = l == 3 ? last_chan_of : wide ? wide_chan_of : hidden_chan_of;
    if (wide) return {wide_mt(l), f32 ? Geo32<true>::groups(l) : wide_ks(l), chan};
    return {Geo32<false>::mt(l), f32 ? Geo32<false>::groups(l) : 1, chan};
}

// Matrix-core weight fragments of layer l: [mt][tap][ks][lane][E] with E = 8 16-bit or 4 fp32 elements;
// element j of a lane is the weight of out-channel chan(mt, lane & 15) at in-position 4E ks + E (lane>>4) + j
// (layer 1: the 24|25 inputs, pos_emb moved to slot 24; hidden layers: position = channel).  F16X3 holds a
// hi|lo pair per ks block, [ks][hi|lo][lane][8], w = hi + lo with hi = f16(w), lo = f16(w - hi).
std::vector<char> pack_frags(const HostWeights& hw, int l, const FragGeo& g, Elem el) {
    const int E = el == EL_F32 ? 4 : 8, parts = el == EL_F16X3 ? 2 : 1;
    std::vector<char> out((size_t)g.mt * kTaps * g.ks * parts * 64 * E * (el == EL_F32 ? 4 : 2));
    uint16_t* h = reinterpret_cast<uint16_t*>(out.data());
    _Float16* h3 = reinterpret_cast<_Float16*>(out.data());
    float* f = reinterpret_cast<float*>(out.data());
    for (int mt = 0; mt < g.mt; ++mt)
        for (int k = 0; k < kTaps; ++k)
            for (int ks = 0; ks < g.ks; ++ks)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < E; ++j) {
                        const float v = hw.at(l, g.chan(mt, lane & 15), 4 * E * ks + E * (lane >> 4) + j, k, true);
                        const size_t at = ((((size_t)mt * kTaps + k) * g.ks + ks) * parts * 64 + lane) * E + j;
                        switch (el) {
                            case EL_BF16: h[at] = f32_to_bf16(v); break;
                            case EL_F16: h[at] = f32_to_f16(v); break;
                            case EL_F16X3:
                                h3[at] = (_Float16)v;
                                h3[at + 64 * 8] = (_Float16)(v - (float)h3[at]);
                                break;
                            default: f[at] = v;
                        }
                    }
    return out;
}

// Layer-1 fragments of the persistent 16-bit kernel for a model without pos_emb (kernel_mfma16.h, PK): the 5 x 24
// operands of a frame are contiguous in its unpadded image, so the k dimension is the flat index 24 tap + channel
// in kL1Steps steps of 32, [mt][step][lane][8]; positions 120..127 lie over the next row's channels: zero weights.
std::vector<char> pack_frags_l1_flat(const HostWeights& hw, const FragGeo& g, Elem el) {
    std::vector<char> out((size_t)g.mt * kL1Steps * 64 * 8 * 2);
    uint16_t* h = reinterpret_cast<uint16_t*>(out.data());
    for (int mt = 0; mt < g.mt; ++mt)
        for (int ks = 0; ks < kL1Steps; ++ks)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int f = 32 * ks + 8 * (lane >> 4) + j;
                    const float v = f < kTaps * kInCh ? hw.at(0, g.chan(mt, lane & 15), f % kInCh, f / kInCh, true) : 0.f;
                    h[(((size_t)mt * kL1Steps + ks) * 64 + lane) * 8 + j] = el == EL_BF16 ? f32_to_bf16(v) : f32_to_f16(v);
                }
    return out;
}

// bias of layer l in the fragments' out-slot order: [mt][q][4] fp32
std::vector<float> pack_bias(const HostWeights& hw, int l, const FragGeo& g) {
    std::vector<float> b((size_t)g.mt * 16);
    for (int mt = 0; mt < g.mt; ++mt)
        for (int q = 0; q < 4; ++q)
            for (int r = 0; r < 4; ++r) b[(mt * 4 + q) * 4 + r] = hw.bias(l, g.chan(mt, 4 * q + r));
    return b;
}

int pack_all(b2h_model* m, const HostWeights& hw) {
    m->w_absmax = 0.f;
    for (int l = 0; l < 4; ++l) m->w_absmax = absmax_of(hw.b[l], absmax_of(hw.w[l], m->w_absmax));
    // ---- VALU layout: w[k][i][opad], reference channel order
    for (int l = 0; l < 4; ++l) {
        const int opad = round_up(m->cout[l], 8), cin = m->cin[l];
        std::vector<float> w((size_t)kTaps * cin * opad, 0.f), b(opad, 0.f);
        for (int k = 0; k < kTaps; ++k)
            for (int i = 0; i < cin; ++i)
                for (int o = 0; o < m->cout[l]; ++o)
                    w[((size_t)k * cin + i) * opad + o] = hw.at(l, o, i, k, false);
        for (int o = 0; o < m->cout[l]; ++o) b[o] = hw.b[l][o];
        int rc = m->valu_w[l].upload(w.data(), w.size() * 4);
        if (rc) return rc;
        rc = m->valu_b[l].upload(b.data(), b.size() * 4);
        if (rc) return rc;
        m->vp.L[l] = ValuLayer{(const float*)m->valu_w[l].p, (const float*)m->valu_b[l].p, cin,
                               m->cout[l], opad};
    }
    {
        int as = round_up(m->C, 8);
        if (as < m->cin[0]) as = m->cin[0];
        m->vp.act_stride = as | 1;
        int wb = 0;
        for (int l = 0; l < 4; ++l) wb = std::max(wb, m->vp.L[l].cin * m->vp.L[l].opad); // one tap at a time
        m->vp.wbuf_floats = wb;
        m->vp.pos_emb = m->pos_emb;
    }
    if (m->C > kMfmaWideWidth) return B2H_OK; // 65..128 channels: the VALU kernel only

    // ---- MFMA layouts: the wave-per-chunk kernels (<= 32 channels: bf16 / f16 run in the persistent kernel)
    const bool wide = m->C > kMfmaWidth;
    int rc;
    for (int l = 0; l < 4; ++l) {
        const std::vector<float> b = pack_bias(hw, l, frag_geo(wide, l, false));
        if ((rc = m->bias[l].upload(b.data(), b.size() * 4))) return rc;
    }
    for (int el = wide ? EL_BF16 : EL_F16X3; el < kElems; ++el) {
        Packed& P = m->pk[el];
        for (int l = 0; l < 4; ++l) {
            const std::vector<char> w = pack_frags(hw, l, frag_geo(wide, l, el == EL_F32), (Elem)el);
            if ((rc = P.w[l].upload(w.data(), w.size()))) return rc;
            P.mp.w[l] = P.w[l].p;
            P.mp.bias[l] = (const float*)m->bias[l].p;
        }
        P.mp.pos_emb = m->pos_emb;
    }
    if (wide) return B2H_OK;
    for (int el : {EL_BF16, EL_F16}) { // the persistent kernel's LDS image
        std::vector<char> img(kPacked16, 0);
        for (int l = 0; l < 4; ++l) {
            const FragGeo g = frag_geo(false, l, false);
            const bool flat = l == 0 && !m->pos_emb; // 24 inputs: layer 1 reads the unpadded image
            const std::vector<char> w = flat ? pack_frags_l1_flat(hw, g, (Elem)el) : pack_frags(hw, l, g, (Elem)el);
            const std::vector<float> b = pack_bias(hw, l, g);
            std::memcpy(img.data() + kWLayerOff16[l], w.data(), w.size());
            std::memcpy(img.data() + kBiasOff16[l], b.data(), b.size() * 4);
        }
        if ((rc = m->img16[el].upload(img.data(), img.size()))) return rc;
    }
    if (!m->pools.p) { // once per model: a later weight replacement must not touch the words of a running launch
        const std::vector<char> zeros((size_t)kPoolSlots * kPoolSlotBytes, 0);
        if ((rc = m->pools.upload(zeros.data(), zeros.size()))) return rc;
    }
    return B2H_OK;
}

int resolve_kernel(const b2h_model* m, int kernel) {
    // AUTO = the faster of the two exact-fp32 kernels (profiles/r2_bf16/widths_8192x200.txt): the
    // matrix-core kernel costs the same at every width of its geometry (<= 32: 2.66 G frames/s,
    // 33..64: 0.77 G), the VALU kernel's cost grows with the width and is ahead only just above the
    // geometry step (0.88 G at 33 channels, level at 40) and for the narrowest models (3.08 G at 8
    // channels, 2.51 G at 10)
    if (kernel == B2H_KERNEL_AUTO)
        return (m->C <= 8 || (m->C > kMfmaWidth && m->C < 40) || m->C > kMfmaWideWidth) ? B2H_KERNEL_F32_VALU
                                                                                          : B2H_KERNEL_F32_MFMA;
    return kernel;
}

bool kernel_ok(const b2h_model* m, int k) {
    switch (k) {
        case B2H_KERNEL_F32_VALU: return m->C <= kMaxWidth;
        case B2H_KERNEL_F32_MFMA:
        case B2H_KERNEL_BF16_MFMA:
        case B2H_KERNEL_F16_MFMA: return m->C <= kMfmaWideWidth; // > 32 channels: the wide kernels
        case B2H_KERNEL_F16X3_MFMA: return m->C <= kMfmaWideWidth && (!m->has_weights || m->w_absmax < kF16Max);
        default: return false;
    }
}

// ---- ConvModel dispatch
// VALU kernel by width: <= 56, 57..104, 105..128 channels (kernel_valu.h: unrolled in-channel loop, three work
// items per thread)
using ValuKernel = void (*)(const float*, float*, int, int, ValuParams, FusedArgs);
constexpr ValuKernel kValuTiers[] = {b2h_fwd_f32_valu<false>, b2h_fwd_f32_valu<true>, b2h_fwd_f32_valu<true, 3>};

// The wave-per-chunk matrix-core kernels, one row per kernel variant and geometry.
using ChunkKernel = void (*)(const float*, float*, int, int, int, int64_t, MfmaParams, FusedArgs);
struct ChunkVariant {
    int kernel;               // B2H_KERNEL_*
    bool wide;                // 33..64 channels
    ChunkKernel plain, fused; // the plain instantiation carries no transform code at all
    int lds;                  // bytes per workgroup
    Elem packed;              // b2h_model::pk entry it reads
    int wgs_per_cu;           // workgroups per CU (__launch_bounds__), for the chunk-length rule
    const char* name;         // b2h_kernel_name
};
constexpr ChunkVariant kChunkVariants[] = {
    {B2H_KERNEL_F32_MFMA, false, b2h_fwd_mfma_f32<false, false>, b2h_fwd_mfma_f32<true, false>,
     kWavesPerBlock * Geo32<false>::kImg, EL_F32, 2, "b2h_fwd_mfma_f32<false, false>"},
    {B2H_KERNEL_F32_MFMA, true, b2h_fwd_mfma_f32<false, true>, b2h_fwd_mfma_f32<true, true>,
     kWavesPerBlock * Geo32<true>::kImg, EL_F32, 1, "b2h_fwd_mfma_f32<false, true>"},
    {B2H_KERNEL_F16X3_MFMA, false, b2h_fwd_mfma_f16x3<false>, b2h_fwd_mfma_f16x3<true>,
     kWavesPerBlock * 2 * kImg3, EL_F16X3, 2, "b2h_fwd_mfma_f16x3<false>"}, // hi + lo images = the fp32 image's bytes
    {B2H_KERNEL_F16X3_MFMA, true, b2h_fwd_mfma_f16x3w<false>, b2h_fwd_mfma_f16x3w<true>,
     kWavesPerBlock * 2 * kImg3W, EL_F16X3, 1, "b2h_fwd_mfma_f16x3w<false>"},
    {B2H_KERNEL_BF16_MFMA, true, b2h_fwd_mfma16w<PREC_BF16, false>, b2h_fwd_mfma16w<PREC_BF16, true>,
     kWavesPerBlock * kImgW, EL_BF16, 2, "b2h_fwd_mfma16w<1, false>"},
    {B2H_KERNEL_F16_MFMA, true, b2h_fwd_mfma16w<PREC_F16, false>, b2h_fwd_mfma16w<PREC_F16, true>,
     kWavesPerBlock * kImgW, EL_F16, 2, "b2h_fwd_mfma16w<2, false>"},
};

// nullptr: the VALU kernel, or the persistent 16-bit kernel (bf16 / f16 at <= 32 channels)
const ChunkVariant* chunk_variant(int k, bool wide) {
    for (const ChunkVariant& v : kChunkVariants)
        if (v.kernel == k && v.wide == wide) return &v;
    return nullptr;
}

// The persistent 16-bit kernel (kernel_mfma16.h): [STREAM][f16][FUSED]
using Kernel16 = void (*)(const float*, float*, int, int, int, int64_t, const void*, int, FusedArgs, Sched16);
constexpr Kernel16 kFwd16[2][2][2] = {
    {{b2h_fwd_mfma16<PREC_BF16, false, false>, b2h_fwd_mfma16<PREC_BF16, true, false>},
     {b2h_fwd_mfma16<PREC_F16, false, false>, b2h_fwd_mfma16<PREC_F16, true, false>}},
    {{b2h_fwd_mfma16<PREC_BF16, false, true>, b2h_fwd_mfma16<PREC_BF16, true, true>},
     {b2h_fwd_mfma16<PREC_F16, false, true>, b2h_fwd_mfma16<PREC_F16, true, true>}},
};

int set_conv_kernel_attributes() {
    static OncePerDevice once;
    return once([] {
        int rc = B2H_OK;
        for (ValuKernel k : kValuTiers)
            if ((rc = raise_lds_cap(k))) return rc;
        for (const ChunkVariant& v : kChunkVariants)
            if ((rc = raise_lds_cap(v.plain)) || (rc = raise_lds_cap(v.fused))) return rc;
        for (const auto& by_prec : kFwd16)
            for (const auto& by_fused : by_prec)
                for (Kernel16 k : by_fused)
                    if ((rc = raise_lds_cap(k))) return rc;
        return rc;
    });
}

// Work distribution of the persistent kernel (Sched16): with >= 256 chunks per workgroup the launch is DYNAMIC
// -- waves claim runs of two consecutive chunks from a device-wide counter, so the chip walks through x and y as
// one front (kernel_mfma16.h).  The counter lives in this stream's slot; no slot (more than kPoolSlots streams),
// a stream under capture (a graph may be replayed on any stream, concurrently with this one) or
// hipStreamPerThread (one handle value for a different stream in every host thread, whose launches would share
// one counter and skip chunks) means a STATIC launch: nullptr.
unsigned* pool_slot(b2h_model* m, hipStream_t st) {
    if (!m->pools.p || st == hipStreamPerThread) return nullptr;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusActive; }
    if (cap != hipStreamCaptureStatusNone) return nullptr;
    std::lock_guard<std::mutex> lock(m->pool_mu);
    size_t slot = 0;
    while (slot < m->pool_streams.size() && m->pool_streams[slot] != st) ++slot;
    if (slot == m->pool_streams.size() && slot < (size_t)kPoolSlots) m->pool_streams.push_back(st);
    if (slot >= (size_t)kPoolSlots) return nullptr;
    return reinterpret_cast<unsigned*>(static_cast<char*>(m->pools.p) + slot * kPoolSlotBytes);
}

// ConvModel shape rules, shared by b2h_forward and the training entry points
int check_shape(const b2h_model* m, int64_t B, int64_t T) {
    if (B < 0 || T < 1) return fail(B2H_ERR_SHAPE, "expected B >= 0 and T >= 1");
    if (T > (1 << 24)) return fail(B2H_ERR_SHAPE, "T too large");
    if (m->pos_emb && T != 100)
        return fail(B2H_ERR_SHAPE, "pos_emb model requires T == 100 (LinearPositionalEmbedding max_len, "
                                   "HandPoseModels.py:23,78-84)");
    return B2H_OK;
}

// x (B, T, 24) and y (B, T, 42) of a ConvModel launch with B >= 1: 16-B vector loads of x rows (96 B each)
// and 8-B granular stores of y rows (168 B each)
int check_xy(const b2h_model* m, const float* x, const float* y, int64_t B, int64_t T) {
    if (!x || !y) return fail(B2H_ERR_INVALID, "x / y is NULL");
    if (int rc = check_device(m->device)) return rc;
    if (misaligned(x, 16) || misaligned(y, 16))
        return fail(B2H_ERR_INVALID, "x and y must be 16-byte aligned (hipMalloc / torch allocations are)");
    if (overlaps(x, (size_t)B * T * kInCh * 4, y, (size_t)B * T * kOutCh * 4)) return fail(B2H_ERR_INVALID, "x and y overlap");
    return B2H_OK;
}

int launch(b2h_model* m, const float* x, float* y, int64_t B, int64_t T, int kernel,
           const FusedArgs& fa, hipStream_t st) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    if (!m->has_weights) return fail(B2H_ERR_NO_WEIGHTS, "b2h_forward before b2h_load_weights");
    if (int rc = check_shape(m, B, T)) return rc;
    if (B == 0) return B2H_OK;
    if (int rc = check_xy(m, x, y, B, T)) return rc;
    if ((fa.flags & kPostMask) && !fa.n_frames)
        return fail(B2H_ERR_INVALID, "B2H_POST_MASK_TAIL needs n_frames");
    const int k = resolve_kernel(m, kernel);
    if (!kernel_ok(m, k)) {
        if (k == B2H_KERNEL_F16X3_MFMA && m->C <= kMfmaWideWidth)
            return fail(B2H_ERR_UNSUPPORTED, "F16X3 kernel: a weight or bias is outside the f16 range (|w| >= 65504 or "
                                             "not finite); use the exact fp32 kernel");
        return fail(B2H_ERR_UNSUPPORTED, "kernel variant does not support conv_channels=" + std::to_string(m->C) +
                                             " (matrix-core kernels: <= 64; exact fp32 VALU kernel: <= 128)");
    }
    const bool fused = fa.flags != 0;
    const ChunkVariant* v = chunk_variant(k, m->C > kMfmaWidth);

    if (k == B2H_KERNEL_F32_VALU) {
        const int tiles = (int)((T + kValuTile - 1) / kValuTile);
        const int64_t grid = B * tiles;
        if (grid > 0x7fffffff) return fail(B2H_ERR_SHAPE, "B*T too large for one launch");
        const size_t lds = ((size_t)2 * kValuRows * m->vp.act_stride + m->vp.wbuf_floats) * 4;
        hipLaunchKernelGGL(kValuTiers[m->C > 104 ? 2 : m->C > 56 ? 1 : 0], dim3((unsigned)grid), dim3(256), lds, st, x,
                           y, (int)T, tiles, m->vp, fa);
    } else if (v) {
        // chunk length of the wave-per-chunk kernels: 112 frames (the LDS image's capacity) unless
        // that leaves most of the chip's wave slots idle (1 or 2 workgroups x 4 waves per CU); then 64 or
        // 32 frames, paying the +-8-frame halo recompute for parallelism.  Any chunking computes
        // bit-identical frames.
        int chunk_len = kChunk;
        const int64_t slots = (int64_t)m->num_cus * v->wgs_per_cu * kWavesPerBlock;
        for (int cand : {64, 32}) {
            if (B * ((T + chunk_len - 1) / chunk_len) * 2 >= slots) break;
            chunk_len = cand;
        }
        const int cps = (int)((T + chunk_len - 1) / chunk_len);
        // (equal chunks -- T = 200 as 100 + 100 instead of 112 + 88 -- measured 3.9 % SLOWER in f16x3 and 1.6 %
        // in exact fp32, same-process A/B, profiles/r3_f16x3/ab_equal_chunks.txt: not done)
        const int64_t nchunks = B * cps;
        const int64_t grid = (nchunks + kWavesPerBlock - 1) / kWavesPerBlock;
        if (grid > 0x7fffffff) return fail(B2H_ERR_SHAPE, "B*T too large for one launch");
        hipLaunchKernelGGL(fused ? v->fused : v->plain, dim3((unsigned)grid), dim3(64 * kWavesPerBlock), v->lds, st, x,
                           y, (int)T, cps, chunk_len, nchunks, m->pk[v->packed].mp, fa);
    } else {
        // persistent kernel: one 512-thread workgroup per CU
        // Chunk length: whole sequences (<= 208 frames) or 192-frame chunks keep the halo
        // recompute at zero / 8 %.  When that leaves most of the chip's 2048 wave slots idle
        // (small batches) shorter chunks trade halo work for parallelism; every chunking
        // computes bit-identical frames.
        int TT = (T <= kChunkWhole16) ? kChunkWhole16 : kChunkSplit16;
        int64_t nch = B * ((T + TT - 1) / TT);
        const int64_t slots = (int64_t)m->num_cus * kWaves16;
        for (int cand : {96, 48}) {
            if (nch * 2 >= slots || T <= cand) break;
            TT = cand;
            nch = B * ((T + TT - 1) / TT);
        }
        const int cps16 = (int)((T + TT - 1) / TT);
        const unsigned grid16 = (unsigned)std::min<int64_t>(m->num_cus, nch);
        if (nch >= 0x7fffffff) return fail(B2H_ERR_SHAPE, "B*T too large for one launch");
        Sched16 sched{nullptr, 2};
        if (nch / grid16 >= kPoolMinChunks) sched.pool = pool_slot(m, st);
        const bool f16 = k == B2H_KERNEL_F16_MFMA;
        // streaming cache policy (kernel_mfma.h: kLdStream / kStStream) from 1 MiB of traffic up
        const bool stream = B * T * (int64_t)((kInCh + kOutCh) * 4) >= (1 << 20);
        hipLaunchKernelGGL(kFwd16[stream][f16][fused], dim3(grid16), dim3(64 * kWaves16), kLdsAlloc16, st, x, y, (int)T,
                           cps16, TT, nch, m->img16[f16].p, m->pos_emb, fa, sched);
    }
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

} // namespace

// ---- TransformerEnc ---------------------------------------------------------------------
// One stage blob of the chain kernel: weight fragments of <= 128 outputs + bias/gamma/beta.
struct TencBlob {
    DevBuf buf;   // fp32 fragments (k-groups of 16)
    DevBuf buf16; // f16 hi + lo fragments (k-groups of 32), B2H_TENC_F16X3
    int mtiles = 0, kgroups = 0, kgroups32 = 0, nout = 0;
};

// One torch.nn.TransformerEncoderLayer (post-norm, ReLU): attn_out carries norm1, ff2 carries norm2.
struct EncLayer {
    TencBlob q, k, v, attn_out, ff1, ff2;
    TencBlob qkv_head[kTencHeads]; // rows of Q_h, K_h, V_h of in_proj_weight: the projection inside b2h_attn_qkv_h3
};

// Floats of its twelve tensors in state_dict order: self_attn in_proj weight, bias; out_proj; linear1; linear2;
// norm1; norm2 (d_model = dim_feedforward = 128).  A decoder layer is made of the same pieces.
constexpr size_t kDD = (size_t)kTencD * kTencD;
constexpr size_t kEncLayerFloats[12] = {3 * kDD, 3 * kTencD, kDD, kTencD, kDD, kTencD, kDD, kTencD, kTencD, kTencD, kTencD, kTencD};

struct b2h_tenc {
    int nlayers = 0, max_len = 0, device = 0;
    bool has_weights = false;
    int kernel = B2H_TENC_F32;
    int train_kernel = B2H_TRAIN_VALU; // b2h_tenc_set_train_kernel
    int train_linear = B2H_TRAIN_VALU; // b2h_tenc_set_train_linear
    float w_absmax = 0.f; // largest |parameter| (NaN counts as inf): B2H_TENC_F16X3 needs < 65504
    // floats of the 5 + 12*nlayers tensors in the order of b2h_tenc_load_weights: pe, pose2hidden_projection, the
    // layers, hidden2pose_projection
    std::vector<size_t> sizes;
    DevBuf pe;
    TencBlob in_proj, out_proj;
    int num_cus = 256;
    std::vector<EncLayer> layers;
};

namespace {

// rows [r0, r0 + nout) of W (*, k) row-major fp32 -> [mt][g][lane][4] with
// W[r0 + 16mt + (lane&15)][16g + 4(lane>>4) + j], followed by bias, gamma, beta (128 each)
// kpad >= k / mpad >= nout (0 = none): the fragment grid is laid out for that many inputs / outputs, the surplus zero,
// so that a Linear of another width runs one of the GEMM shapes the chain kernel has (tpt_front_kpad, kTptHeadMpad)
int pack_blob(TencBlob& B, const float* w, const float* b, int r0, int nout, int k, const float* gamma,
              const float* beta, int kpad = 0, int mpad = 0) {
    B.kgroups = (std::max(k, kpad) + 15) / 16;
    B.mtiles = (std::max(nout, mpad) + 15) / 16;
    B.nout = nout;
    const size_t nw = (size_t)B.mtiles * B.kgroups * 64 * 4;
    std::vector<float> blob(nw + kStageParams, 0.f);
    for (int mt = 0; mt < B.mtiles; ++mt)
        for (int g = 0; g < B.kgroups; ++g)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    const int o = 16 * mt + (lane & 15), kk = 16 * g + 4 * (lane >> 4) + j;
                    if (o < nout && kk < k)
                        blob[(((size_t)mt * B.kgroups + g) * 64 + lane) * 4 + j] = w[(size_t)(r0 + o) * k + kk];
                }
    for (int o = 0; o < nout; ++o) blob[nw + o] = b[r0 + o];
    if (gamma) std::memcpy(blob.data() + nw + kTencD, gamma, kTencD * 4);
    if (beta) std::memcpy(blob.data() + nw + 2 * kTencD, beta, kTencD * 4);
    int rc = B.buf.upload(blob.data(), blob.size() * 4);
    if (rc) return rc;
    // f16 hi/lo fragments for v_mfma_f32_16x16x32_f16: [part][mt][g][lane][8] with k-slot (g, q, j)
    // = input feature 32g + 16(j>>2) + 4q + (j&3) (kernel_tenc.h), then the same fp32 parameters
    B.kgroups32 = (std::max(k, kpad) + 31) / 32;
    const size_t nh = (size_t)B.mtiles * B.kgroups32 * 64 * 8; // halves per part
    std::vector<_Float16> frag(2 * nh, (_Float16)0.f);
    for (int mt = 0; mt < B.mtiles; ++mt)
        for (int g = 0; g < B.kgroups32; ++g)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int o = 16 * mt + (lane & 15), kk = 32 * g + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3);
                    if (o < nout && kk < k) {
                        const float x = w[(size_t)(r0 + o) * k + kk];
                        const _Float16 hi = (_Float16)x;
                        const size_t at = (((size_t)mt * B.kgroups32 + g) * 64 + lane) * 8 + j;
                        frag[at] = hi;
                        frag[nh + at] = (_Float16)(x - (float)hi);
                    }
                }
    std::vector<char> blob16(2 * nh * 2 + kStageParams * 4);
    std::memcpy(blob16.data(), frag.data(), 2 * nh * 2);
    std::memcpy(blob16.data() + 2 * nh * 2, blob.data() + nw, kStageParams * 4);
    return B.buf16.upload(blob16.data(), blob16.size());
}

// The per-head blobs [Q_h | K_h | V_h] of one attention block: rows 32 hd .. of each third of its in_proj weight
// (384, 128) and bias (384), for the projection inside b2h_attn_qkv_h3 / b2h_attn_cross_h3
int pack_qkv_heads(TencBlob (&heads)[kTencHeads], const float* w, const float* b) {
    const int D = kTencD;
    for (int hd = 0; hd < kTencHeads; ++hd) {
        std::vector<float> wh((size_t)3 * kTencHd * D), bhd((size_t)3 * kTencHd);
        for (int part = 0; part < 3; ++part)
            for (int r = 0; r < kTencHd; ++r) {
                std::memcpy(&wh[((size_t)part * kTencHd + r) * D], &w[((size_t)part * D + hd * kTencHd + r) * D], D * 4);
                bhd[part * kTencHd + r] = b[part * D + hd * kTencHd + r];
            }
        if (int rc = pack_blob(heads[hd], wh.data(), bhd.data(), 0, 3 * kTencHd, D, nullptr, nullptr)) return rc;
    }
    return B2H_OK;
}

// One launch of the chain kernel under construction: the rows that enter, then the stages in order.  h3 selects the
// f16 hi + lo fragments (k-groups of 32) and b2h_tenc_chain<true>, otherwise the fp32 ones (k-groups of 16).
struct Chain {
    bool h3 = false;
    ChainArgs a{};
    // (n, ldx) rows entering the chain, with the (n, 128) residual rows of a leading ST_RESLN_GLOBAL stage
    void rows(const float* x, int ldx, const float* res, int64_t n) {
        a.x = x; a.ldx = ldx; a.kgroups0 = (ldx + 15) / 16; a.kvalid = ldx; a.T = 1;
        a.res = res; a.n = n;
    }
    void add(const TencBlob& B, int type, float* out, int ldo = kTencD) {
        a.st[a.nstages++] = h3 ? ChainStage{(const float*)B.buf16.p, out, type, B.mtiles, B.kgroups32, ldo, B.nout, 2 * B.mtiles * B.kgroups32 * 64}
                               : ChainStage{(const float*)B.buf.p, out, type, B.mtiles, B.kgroups, ldo, B.nout, B.mtiles * B.kgroups * 64};
    }
    void add_qkv(const TencBlob& q, const TencBlob& k, const TencBlob& v, float* QKV) {
        add(q, ST_STORE, QKV, 3 * kTencD);
        add(k, ST_STORE, QKV + kTencD, 3 * kTencD);
        add(v, ST_STORE, QKV + 2 * kTencD, 3 * kTencD);
    }
    // out_proj +res LN1 -> linear1 ReLU -> linear2 +res LN2 -> residual stream `xs` (or nullptr: the rows stay in
    // registers for the stages that follow) [+ the Q, K, V rows of the layer `next`]
    void add_layer_tail(const TencBlob& out_proj, const TencBlob& ff1, const TencBlob& ff2, float* xs, const EncLayer* next,
                        float* QKV) {
        add(out_proj, ST_RESLN_GLOBAL, nullptr);
        add(ff1, ST_RELU, nullptr);
        add(ff2, ST_RESLN_REG, xs);
        if (next) add_qkv(next->q, next->k, next->v, QKV);
    }
    void launch(int num_cus, hipStream_t st) const {
        // persistent: one workgroup per CU (134 KB of LDS each) walks over the 128-row blocks
        const int64_t blocks = std::min<int64_t>((a.n + 16 * kLinWaves - 1) / (16 * kLinWaves), num_cus);
        hipLaunchKernelGGL(h3 ? b2h_tenc_chain<true> : b2h_tenc_chain<false>, dim3((unsigned)blocks), dim3(64 * kLinWaves),
                           (size_t)kChainLdsBytes, st, a);
    }
};

// f16x3 self-attention by query tiles, [nt - 1] with nt = ceil(T / 16) <= 8: b2h_attn_qkv_h3 projects Q, K, V itself
using AttnQkvKernel = void (*)(AttnQkvArgs);
constexpr AttnQkvKernel kAttnQkvH3[kAttnMaxTiles] = {b2h_attn_qkv_h3<1>, b2h_attn_qkv_h3<2>, b2h_attn_qkv_h3<3>,
                                                     b2h_attn_qkv_h3<4>, b2h_attn_qkv_h3<5>, b2h_attn_qkv_h3<6>,
                                                     b2h_attn_qkv_h3<7>, b2h_attn_qkv_h3<8>};
// f16x3 cross-attention (TextPoseTransformer) by KEY tiles, [nk - 1] with nk = ceil(S / 16); the block size carries
// the query tiles
using AttnCrossH3Kernel = void (*)(AttnCrossArgs);
constexpr AttnCrossH3Kernel kAttnCrossH3[kAttnMaxTiles] = {b2h_attn_cross_h3<1>, b2h_attn_cross_h3<2>, b2h_attn_cross_h3<3>,
                                                           b2h_attn_cross_h3<4>, b2h_attn_cross_h3<5>, b2h_attn_cross_h3<6>,
                                                           b2h_attn_cross_h3<7>, b2h_attn_cross_h3<8>};
// Attention over described rows (AttnSrc) by key tiles, [nk - 1]: fp32 up to 128 query rows with nk = ceil(Tk / 16) (the
// block size carries the query tiles; row [1] for launches with as many query tiles as key tiles); beyond
// (kernel_attn_long.h), both arithmetics, nk = key tiles per key block
using AttnRowsKernel = void (*)(AttnSrc, float*, int, int);
constexpr AttnRowsKernel kAttnF32[2][kAttnMaxTiles] = {
    {b2h_attn_f32<1, false>, b2h_attn_f32<2, false>, b2h_attn_f32<3, false>, b2h_attn_f32<4, false>, b2h_attn_f32<5, false>,
     b2h_attn_f32<6, false>, b2h_attn_f32<7, false>, b2h_attn_f32<8, false>},
    {b2h_attn_f32<1, true>, b2h_attn_f32<2, true>, b2h_attn_f32<3, true>, b2h_attn_f32<4, true>, b2h_attn_f32<5, true>,
     b2h_attn_f32<6, true>, b2h_attn_f32<7, true>, b2h_attn_f32<8, true>}};
constexpr AttnRowsKernel kAttnLongF32[kAttnMaxTiles] = {b2h_attn_long_f32<1>, b2h_attn_long_f32<2>, b2h_attn_long_f32<3>,
                                                        b2h_attn_long_f32<4>, b2h_attn_long_f32<5>, b2h_attn_long_f32<6>,
                                                        b2h_attn_long_f32<7>, b2h_attn_long_f32<8>};
// The two fp32 kernels with a key length per sequence (a key-padding mask): instantiations of
// their own, so that the ones above stay what they were
using AttnRowsKlKernel = void (*)(AttnSrc, float*, int, int, const int64_t*);
constexpr AttnRowsKlKernel kAttnF32Kl[2][kAttnMaxTiles] = {
    {b2h_attn_klen_f32<1, false>, b2h_attn_klen_f32<2, false>, b2h_attn_klen_f32<3, false>, b2h_attn_klen_f32<4, false>,
     b2h_attn_klen_f32<5, false>, b2h_attn_klen_f32<6, false>, b2h_attn_klen_f32<7, false>, b2h_attn_klen_f32<8, false>},
    {b2h_attn_klen_f32<1, true>, b2h_attn_klen_f32<2, true>, b2h_attn_klen_f32<3, true>, b2h_attn_klen_f32<4, true>,
     b2h_attn_klen_f32<5, true>, b2h_attn_klen_f32<6, true>, b2h_attn_klen_f32<7, true>, b2h_attn_klen_f32<8, true>}};
constexpr AttnRowsKlKernel kAttnLongF32Kl[kAttnMaxTiles] = {
    b2h_attn_long_klen_f32<1>, b2h_attn_long_klen_f32<2>, b2h_attn_long_klen_f32<3>, b2h_attn_long_klen_f32<4>,
    b2h_attn_long_klen_f32<5>, b2h_attn_long_klen_f32<6>, b2h_attn_long_klen_f32<7>, b2h_attn_long_klen_f32<8>};
constexpr AttnRowsKernel kAttnLongH3[kAttnMaxTiles] = {b2h_attn_long_h3<1>, b2h_attn_long_h3<2>, b2h_attn_long_h3<3>,
                                                       b2h_attn_long_h3<4>, b2h_attn_long_h3<5>, b2h_attn_long_h3<6>,
                                                       b2h_attn_long_h3<7>, b2h_attn_long_h3<8>};

// The LDS caps of the transformer kernels (inference and training), raised when a TransformerEnc or a
// TextPoseTransformer is created: here, not in a launch, so that every forward is capture-safe from the first one.
int set_tenc_kernel_attributes() {
    static OncePerDevice once;
    return once([]() -> int {
        int rc;
        if ((rc = raise_lds_cap(b2h_tenc_chain<false>, kChainLdsBytes)) || (rc = raise_lds_cap(b2h_tenc_chain<true>, kChainLdsBytes)))
            return rc;
        for (int nt = 1; nt <= kAttnMaxTiles; ++nt)
            if ((rc = raise_lds_cap(kAttnQkvH3[nt - 1], attn_qkv_lds_bytes(nt))) ||
                (rc = raise_lds_cap(kAttnCrossH3[nt - 1], attn_qkv_lds_bytes(nt))) ||
                (rc = raise_lds_cap(kAttnLongF32[nt - 1], attn_long_f32_lds_bytes(nt))) ||
                (rc = raise_lds_cap(kAttnLongF32Kl[nt - 1], attn_long_f32_lds_bytes(nt))) ||
                (rc = raise_lds_cap(kAttnLongH3[nt - 1], attn_long_h3_lds_bytes(nt))))
                return rc;
        if ((rc = raise_lds_cap(b2h_tt_sdpa)) || (rc = raise_lds_cap(b2h_tt_sdpa_bwd))) return rc;
        if ((rc = raise_lds_cap(b2h_mw_sdpa)) || (rc = raise_lds_cap(b2h_mw_sdpa_bwd))) return rc;
        if ((rc = raise_lds_cap(b2h_lt_sdpa, (int)kLtFwdLds)) || (rc = raise_lds_cap(b2h_lt_sdpa_bwd_kv, (int)kLtBwdKvLds)) ||
            (rc = raise_lds_cap(b2h_lt_sdpa_bwd_q, (int)kLtBwdQLds)))
            return rc;
        if ((rc = raise_lds_cap(b2h_mt_sdpa, (int)kMtFwdLds)) || (rc = raise_lds_cap(b2h_mt_sdpa_bwd_kv, (int)kMtBwdKvLds)) ||
            (rc = raise_lds_cap(b2h_mt_sdpa_bwd_q, (int)kMtBwdQLds)))
            return rc;
        if ((rc = raise_lds_cap(b2h_ml_linear, (int)kMlFwdLds)) || (rc = raise_lds_cap(b2h_ml_linear_dx, (int)kMlDxLds)) ||
            (rc = raise_lds_cap(b2h_ml_linear_dw, (int)kMlDwLds)))
            return rc;
        return B2H_OK;
    });
}

// The persistent grid of the f16x3 attention kernels: one workgroup per CU, bound to a head
// (blockIdx = 8 (4 slot + head) + xcd: 32 per sequence slot)
unsigned attn_h3_grid(int num_cus) { return (unsigned)std::max(32, num_cus / 32 * 32); }

// f16x3 self-attention of B sequences of T <= 128 rows with its projections inside: x (B*T, 128) -> OC (B*T, 128)
void self_attn_h3(const TencBlob (&heads)[kTencHeads], const float* x, float* OC, int64_t B, int T, int num_cus, hipStream_t st) {
    const int nt = (T + 15) / 16;
    AttnQkvArgs qa{};
    qa.x = x; qa.out = OC; qa.T = T; qa.B = B;
    for (int hd = 0; hd < kTencHeads; ++hd) qa.blob[hd] = (const float*)heads[hd].buf16.p;
    hipLaunchKernelGGL(kAttnQkvH3[nt - 1], dim3(attn_h3_grid(num_cus)), dim3(64 * nt), (size_t)attn_qkv_lds_bytes(nt), st, qa);
}

// The operands of the two attentions, inference and training: the chain's [Q | K | V] rows against themselves, and
// the decoder's cross-query rows against the memory's [K | V] rows
AttnSrc self_src(const float* qkv) { return AttnSrc{qkv, 3 * kTencD, 0, qkv, 3 * kTencD, kTencD, 2 * kTencD}; }
AttnSrc cross_src(const float* qc, const float* kv) { return AttnSrc{qc, kTencD, 0, kv, 2 * kTencD, 0, kTencD}; }

// Inference attention of B sequences of Tq query rows over Tk key rows, out (B*Tq, 128).  Tq <= 128 (and Tk <= 128):
// the whole-matrix b2h_attn_f32, one wave per query tile.  That arm is exact fp32 ONLY: f16x3 at T <= 128 keeps its
// fused kernels (self_attn_h3, b2h_attn_cross_h3) and never gets here.  Beyond, both arithmetics (kernel_attn_long.h):
// the query tiles are cut into ceil(tiles / 8) blocks of equal tile count (>= 5 for Tq > 128, which the kernels'
// klen: (B) key lengths on the device or nullptr (fp32 only; the caller refuses f16x3 with lengths).  The launch
// geometry is that of (Tq, Tk) either way.
void attn_rows(hipStream_t st, bool h3, const AttnSrc& src, float* out, int64_t B, int Tq, int Tk, const int64_t* klen) {
    const int ntq = (Tq + 15) / 16, ntk = (Tk + 15) / 16;
    if (ntq <= kAttnMaxTiles) {
        const dim3 grid((unsigned)(B * kTencHeads)), block(64 * ntq);
        if (klen)
            hipLaunchKernelGGL(kAttnF32Kl[ntq == ntk][ntk - 1], grid, block, (size_t)attn_f32_lds_bytes(ntk), st, src, out, Tq,
                               Tk, klen);
        else
            hipLaunchKernelGGL(kAttnF32[ntq == ntk][ntk - 1], grid, block, (size_t)attn_f32_lds_bytes(ntk), st, src, out, Tq, Tk);
        return;
    }
    const int nqb = (ntq + kAttnMaxTiles - 1) / kAttnMaxTiles, wpb = (ntq + nqb - 1) / nqb;
    const int nkb = (ntk + kAttnMaxTiles - 1) / kAttnMaxTiles, nk = (ntk + nkb - 1) / nkb;
    if (klen) {
        hipLaunchKernelGGL(kAttnLongF32Kl[nk - 1], dim3((unsigned)(B * kTencHeads), (unsigned)nqb), dim3(64 * wpb),
                           (size_t)attn_long_f32_lds_bytes(nk), st, src, out, Tq, Tk, klen);
        return;
    }
    hipLaunchKernelGGL(h3 ? kAttnLongH3[nk - 1] : kAttnLongF32[nk - 1], dim3((unsigned)(B * kTencHeads), (unsigned)nqb),
                       dim3(64 * wpb), (size_t)(h3 ? attn_long_h3_lds_bytes(nk) : attn_long_f32_lds_bytes(nk)), st, src, out,
                       Tq, Tk);
}

// Residual stream XA, attention output OC and (fp32 path) the Q, K, V rows of the next attention; QKV is
// nullptr on the f16x3 path, whose attention kernel projects them itself.
struct TencWs {
    float *XA, *OC, *QKV;
};

// src + pe -> pose2hidden_projection (HandPoseModels.py:167-169) -> residual stream [+ layer 0's Q, K, V]
void chain_in(b2h_tenc* m, const float* x, int64_t n, int T, const FusedArgs& fa, const TencWs& ws, hipStream_t st) {
    Chain c{m->kernel == B2H_TENC_F16X3};
    c.rows(x, kInCh, nullptr, n);
    c.a.pe = (const float*)m->pe.p; c.a.T = T;
    c.a.flags = fa.flags & (kPreChest | kPreNorm); c.a.factor = fa.factor; c.a.Tseq = T;
    c.add(m->in_proj, ST_SET, ws.XA);
    if (ws.QKV) c.add_qkv(m->layers[0].q, m->layers[0].k, m->layers[0].v, ws.QKV);
    c.launch(m->num_cus, st);
}

// the layer's tail -> residual stream [+ next layer's Q, K, V] | hidden2pose (:171)
void chain_tail(b2h_tenc* m, int l, float* y, int64_t n, int T, const FusedArgs& fa, const TencWs& ws, hipStream_t st) {
    const EncLayer& L = m->layers[l];
    const bool last = l + 1 == m->nlayers;
    Chain c{m->kernel == B2H_TENC_F16X3};
    c.rows(ws.OC, kTencD, ws.XA, n);
    c.a.Tseq = T;
    // XA: the next layer's input and residual
    c.add_layer_tail(L.attn_out, L.ff1, L.ff2, last ? nullptr : ws.XA, !last && ws.QKV ? &m->layers[l + 1] : nullptr, ws.QKV);
    if (last) {
        c.add(m->out_proj, ST_STORE, y, kOutCh);
        c.a.flags = fa.flags & (kPostDenorm | kPostMask); c.a.factor = fa.factor; c.a.n_frames = fa.n_frames;
    }
    c.launch(m->num_cus, st);
}

int tenc_launch(b2h_tenc* m, const float* x, float* y, int64_t B, int64_t T, const FusedArgs& fa, void* workspace,
                size_t workspace_bytes, void* stream) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    if (!m->has_weights) return fail(B2H_ERR_NO_WEIGHTS, "b2h_tenc_forward before b2h_tenc_load_weights");
    if (B < 0 || T < 1) return fail(B2H_ERR_SHAPE, "expected B >= 0 and T >= 1");
    if (T > m->max_len)
        return fail(B2H_ERR_SHAPE, "TransformerEnc: T exceeds the positional encoding's max_len (src + pe[:T], "
                                   "HandPoseModels.py:101,167)");
    if (B == 0) return B2H_OK;
    const int64_t n = B * T;
    // grid limits: attention launches B x heads workgroups, the chain n / 128
    if (B * kTencHeads > 0x7fffffff || n / (16 * kLinWaves) >= 0x7fffffff) return fail(B2H_ERR_SHAPE, "batch too large for one launch");
    if (!x || !y || !workspace) return fail(B2H_ERR_INVALID, "NULL pointer");
    if (int rc = check_device(m->device)) return rc;
    if (m->kernel == B2H_TENC_F16X3 && !(m->w_absmax < kF16Max))
        return fail(B2H_ERR_UNSUPPORTED, "B2H_TENC_F16X3: a parameter is outside the f16 range (|w| >= 65504 or not "
                                         "finite); use B2H_TENC_F32");
    if (misaligned(x, 16) || misaligned(workspace, 16)) return fail(B2H_ERR_INVALID, "x and workspace must be 16-byte aligned");
    if (workspace_bytes < b2h_tenc_workspace_bytes(m, B, T)) return fail(B2H_ERR_INVALID, "workspace too small");
    const int nt = (int)((T + 15) / 16);
    if (nt > kAttnMaxTiles) return fail(B2H_ERR_SHAPE, "TransformerEnc: T > 128");
    hipStream_t st = (hipStream_t)stream;
    // f16x3, round 3: the Q, K, V projection runs inside the attention kernel (b2h_attn_qkv_h3), so only the residual
    // stream and the attention output cross HBM between launches (2.5 KB per frame and layer -> 1.25 KB).
    const bool h3 = m->kernel == B2H_TENC_F16X3;
    float* XA = reinterpret_cast<float*>(workspace);
    const TencWs ws{XA, XA + n * kTencD, h3 ? nullptr : XA + 2 * n * kTencD};
    chain_in(m, x, n, (int)T, fa, ws, st);
    for (int l = 0; l < m->nlayers; ++l) { // torch.nn.TransformerEncoderLayer, post-norm, ReLU
        if (h3) self_attn_h3(m->layers[l].qkv_head, ws.XA, ws.OC, B, (int)T, m->num_cus, st);
        else attn_rows(st, false, self_src(ws.QKV), ws.OC, B, (int)T, (int)T, nullptr);
        chain_tail(m, l, y, n, (int)T, fa, ws, st);
    }
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

} // namespace

extern "C" {

int b2h_tenc_create(int ninp, int nhead, int nhid, int nout, int nlayers, int max_len, b2h_tenc** out) {
    if (!out) return fail(B2H_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (ninp != kInCh || nhead != kTencHeads || nhid != kTencD || nout != kOutCh)
        return fail(B2H_ERR_UNSUPPORTED, "TransformerEnc: only ninp=24, nhead=4, nhid=128, nout=42 "
                                         "(infer_utterance.py:99-101) is implemented");
    if (nlayers < 1 || nlayers > 16 || max_len < 1 || max_len > 128)
        return fail(B2H_ERR_UNSUPPORTED, "TransformerEnc: 1 <= nlayers <= 16 and 1 <= max_len <= 128");
    std::unique_ptr<b2h_tenc> m(new b2h_tenc()); // released to the caller only on success
    if (int rc = probe_device(m->device, m->num_cus)) return rc;
    if (int rc = set_tenc_kernel_attributes()) return rc;
    m->nlayers = nlayers;
    m->max_len = max_len;
    m->sizes = {(size_t)max_len * kInCh, (size_t)kTencD * kInCh, (size_t)kTencD};
    for (int l = 0; l < nlayers; ++l) m->sizes.insert(m->sizes.end(), kEncLayerFloats, kEncLayerFloats + 12);
    m->sizes.insert(m->sizes.end(), {(size_t)kOutCh * kTencD, (size_t)kOutCh});
    m->layers.resize(nlayers);
    *out = m.release();
    return B2H_OK;
}

int b2h_tenc_destroy(b2h_tenc* m) {
    delete m;
    return B2H_OK;
}

int b2h_tenc_set_kernel(b2h_tenc* m, int kernel) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    if (kernel != B2H_TENC_F32 && kernel != B2H_TENC_F16X3) return fail(B2H_ERR_INVALID, "unknown TransformerEnc kernel");
    m->kernel = kernel;
    return B2H_OK;
}

int b2h_tenc_load_weights(b2h_tenc* m, const float* const* tensors, int count, int on_device) {
    if (!m || !tensors) return fail(B2H_ERR_INVALID, "NULL argument");
    if (count != (int)m->sizes.size()) return fail(B2H_ERR_INVALID, "expected 5 + 12*nlayers tensors");
    for (int i = 0; i < count; ++i)
        if (!tensors[i]) return fail(B2H_ERR_INVALID, "tensor pointer is NULL");
    const int D = kTencD;
    std::vector<std::vector<float>> h;
    int rc;
    if ((rc = fetch_tensors(tensors, m->sizes, on_device, h)) || (rc = check_device(m->device))) return rc;
    m->w_absmax = 0.f;
    for (int i = 1; i < count; ++i) m->w_absmax = absmax_of(h[i], m->w_absmax); // h[0] is the pe table (|pe| <= 1)
    if ((rc = m->pe.upload(h[0].data(), h[0].size() * 4))) return rc;
    if ((rc = pack_blob(m->in_proj, h[1].data(), h[2].data(), 0, D, kInCh, nullptr, nullptr))) return rc;
    for (int l = 0; l < m->nlayers; ++l) {
        auto& L = m->layers[l];
        const int o = 3 + 12 * l;
        if ((rc = pack_blob(L.q, h[o].data(), h[o + 1].data(), 0, D, D, nullptr, nullptr))) return rc;
        if ((rc = pack_blob(L.k, h[o].data(), h[o + 1].data(), D, D, D, nullptr, nullptr))) return rc;
        if ((rc = pack_blob(L.v, h[o].data(), h[o + 1].data(), 2 * D, D, D, nullptr, nullptr))) return rc;
        if ((rc = pack_qkv_heads(L.qkv_head, h[o].data(), h[o + 1].data()))) return rc;
        if ((rc = pack_blob(L.attn_out, h[o + 2].data(), h[o + 3].data(), 0, D, D, h[o + 8].data(), h[o + 9].data()))) return rc;
        if ((rc = pack_blob(L.ff1, h[o + 4].data(), h[o + 5].data(), 0, D, D, nullptr, nullptr))) return rc;
        if ((rc = pack_blob(L.ff2, h[o + 6].data(), h[o + 7].data(), 0, D, D, h[o + 10].data(), h[o + 11].data()))) return rc;
    }
    const int o = 3 + 12 * m->nlayers;
    if ((rc = pack_blob(m->out_proj, h[o].data(), h[o + 1].data(), 0, kOutCh, D, nullptr, nullptr))) return rc;
    m->has_weights = true;
    return B2H_OK;
}

size_t b2h_tenc_workspace_bytes(const b2h_tenc* m, int64_t B, int64_t T) {
    if (!m || B < 0 || T < 0) return 0;
    return (size_t)B * T * (5 * kTencD) * sizeof(float); // residual stream XA, attention output OC (128 each) + QKV (384)
}

int b2h_tenc_forward(b2h_tenc* m, const float* x, float* y, int64_t B, int64_t T, void* workspace,
                     size_t workspace_bytes, void* stream) {
    FusedArgs fa{0, 1.0f, nullptr};
    return tenc_launch(m, x, y, B, T, fa, workspace, workspace_bytes, stream);
}

int b2h_tenc_forward_fused(b2h_tenc* m, const float* body, float* y, int64_t B, int64_t T, int flags, float factor,
                           const int64_t* n_frames, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_fused(flags, factor)) return rc;
    if ((flags & kPostMask) && !n_frames) return fail(B2H_ERR_INVALID, "B2H_POST_MASK_TAIL needs n_frames");
    FusedArgs fa{flags, factor, n_frames};
    return tenc_launch(m, body, y, B, T, fa, workspace, workspace_bytes, stream);
}

} // extern "C"

// ---- TextPoseTransformer (kernel_tpt.h) -----------------------------------------------------------------------
// torch.nn.Transformer(128, 4, n_enc, n_dec, 128) between a token embedding and the two pose projections
// (HandPoseModels.py:181-230), inference, exact fp32 or f16x3.  Per-frame work is b2h_tenc_chain<H3> by descriptors.
struct b2h_tpt {
    int n_tokens = 0, n_enc = 0, n_dec = 0, device = 0, num_cus = 256;
    int ninp = kInCh, nout = kOutCh; // n_joints*joints_dim in {16, 24, 42, 58}, head width in {8, 24, 42}
    bool has_weights = false;
    int kernel = B2H_TENC_F32;
    int train_kernel = B2H_TRAIN_VALU; // b2h_tpt_set_train_kernel
    int train_linear = B2H_TRAIN_VALU; // b2h_tpt_set_train_linear
    int train_whole = B2H_TRAIN_VALU;  // b2h_tpt_set_train_whole
    float w_absmax = 0.f; // largest |parameter|, the embedding table included (NaN counts as inf): B2H_TENC_F16X3 needs < 65504
    DevBuf table;               // token_embedding.weight (n_tokens, 128)
    DevBuf enc_norm, dec_norm;  // encoder.norm / decoder.norm: gamma (128), beta (128)
    TencBlob in_proj, out_proj; // pose2hidden_projection, hidden2pose_projection
    struct DecLayer : EncLayer {          // q, k, v, attn_out: self_attn, its out_proj carries norm1; ff2 carries norm3
        TencBlob cq, ck, cv, cross_out;   // multihead_attn on the encoder memory; out_proj carries norm2
        TencBlob cross_head[kTencHeads];  // its [Q_h | K_h | V_h] rows: the projections inside b2h_attn_cross_h3
    };
    std::vector<EncLayer> enc;
    std::vector<DecLayer> dec;
};

namespace {

// The geometry lives in the front (pose2hidden_projection) and the head (hidden2pose_projection) only, and both run
// GEMM shapes the chain kernel already has, on zero-padded fragment grids (pack_blob's kpad / mpad):
//   front  ninp 16, 24: two k-groups of 16 (fp32) / one of 32 (f16x3), the default model's shape; rows read in place
//          ninp 42, 58: the 128-input shape of every inner Linear, rows read from a zero-padded 64-float copy
//                       (b2h_item_pad_rows), of which the chain loads k-groups 0..3 and leaves 4..7 zero
//   head   nout 8, 24, 42: three M-tiles; the store's range check keeps it to nout columns.
constexpr int kTptHeadMpad = 48;
int tpt_front_kpad(int ninp) { return ninp <= 32 ? 32 : kTencD; }
bool tpt_padded_rows(const b2h_tpt* m) { return m->ninp > 32; }
int tpt_front_ld(const b2h_tpt* m) { return tpt_padded_rows(m) ? kTptPadLd : m->ninp; }

constexpr int kTptMaxLen = 16 * kAttnMaxTiles; // tokens and frames per sequence: one workgroup holds all keys

// Workspace (floats; Ns = B*S token rows, Nt = B*T frame rows).  Every region is written before it is read; the
// f16x3 path uses MEM, OCs, XT, X1 and OCt only (its attention kernels project Q, K, V themselves):
//   MEM  Ns x 128  encoder residual stream, at the end the memory (after encoder.norm)
//   OCs  Ns x 128  encoder attention output          QKVs Ns x 384  encoder Q | K | V
//   MKV  n_dec x (Ns x 256)  K | V of the memory for each decoder layer's multihead_attn
//   XT   Nt x 128  decoder residual stream           X1   Nt x 128  norm1 output (residual of the cross block)
//   OCt  Nt x 128  attention output (self, cross)    QC   Nt x 128  cross-attention query
//   QKVt Nt x 384  decoder self-attention Q | K | V
//   XP   Nt x 64   the pose rows zero-padded, for ninp in {42, 58} only
constexpr int64_t kTptTokenFloats = 5 * kTencD, kTptTokenLayerFloats = 2 * kTencD, kTptFrameFloats = 7 * kTencD;
struct TptWs {
    float *MEM, *OCs, *QKVs, *MKV, *XT, *X1, *OCt, *QC, *QKVt, *XP;
};
TptWs tpt_ws(void* workspace, int64_t Ns, int64_t Nt, int n_dec) {
    TptWs w;
    w.MEM = reinterpret_cast<float*>(workspace);
    w.OCs = w.MEM + Ns * kTencD;
    w.QKVs = w.OCs + Ns * kTencD;
    w.MKV = w.QKVs + Ns * 3 * kTencD;
    w.XT = w.MKV + Ns * kTptTokenLayerFloats * n_dec;
    w.X1 = w.XT + Nt * kTencD;
    w.OCt = w.X1 + Nt * kTencD;
    w.QC = w.OCt + Nt * kTencD;
    w.QKVt = w.QC + Nt * kTencD;
    w.XP = w.QKVt + Nt * 3 * kTencD;
    return w;
}

// A chain without the item transforms: (n, ldx) rows, optional (n, 128) residual rows
Chain tpt_rows(const float* x, int ldx, const float* res, int64_t n, bool h3 = false) {
    Chain c{h3};
    c.rows(x, ldx, res, n);
    c.a.Tseq = 1; c.a.factor = 1.0f;
    return c;
}

// Floats of the 9 + 12*n_enc + 18*n_dec parameters in the order of b2h_tpt_load_weights.  A decoder layer: two
// attention blocks, linear1 and linear2, three LayerNorms.
std::vector<size_t> tpt_param_floats(const b2h_tpt* m) {
    const size_t D = kTencD;
    const size_t* E = kEncLayerFloats;
    std::vector<size_t> sizes;
    for (int l = 0; l < m->n_enc; ++l) sizes.insert(sizes.end(), E, E + 12);
    sizes.insert(sizes.end(), 2, D);
    for (int l = 0; l < m->n_dec; ++l) {
        sizes.insert(sizes.end(), E, E + 4);
        sizes.insert(sizes.end(), E, E + 8);
        sizes.insert(sizes.end(), 6, D);
    }
    sizes.insert(sizes.end(), 2, D);
    sizes.insert(sizes.end(), {(size_t)m->n_tokens * D, (size_t)m->nout * D, (size_t)m->nout, D * m->ninp, D});
    return sizes;
}

void tpt_layernorm(const DevBuf& gb, float* x, int64_t n, hipStream_t st) {
    const float* g = (const float*)gb.p;
    hipLaunchKernelGGL(b2h_tpt_layernorm, dim3((unsigned)((n + 7) / 8)), dim3(256), 0, st, x, g, g + kTencD, x, n);
}

} // namespace

extern "C" {

int b2h_tpt_create(int n_tokens, int ninp, int nhead, int nhid, int nout, int n_enc_layers, int n_dec_layers,
                   b2h_tpt** out) {
    if (!out) return fail(B2H_ERR_INVALID, "out is NULL");
    *out = nullptr;
    const bool geom = (ninp == 16 || ninp == 24 || ninp == 42 || ninp == 58) && (nout == 8 || nout == 24 || nout == 42);
    if (!geom || nhead != kTencHeads || nhid != kTencD)
        return fail(B2H_ERR_UNSUPPORTED, "TextPoseTransformer: only n_joints*joints_dim in {16, 24, 42, 58}, nout in "
                                         "{8, 24, 42} (run.py:85-104), nhead=4, nhid=128 (run.py:148-151) is implemented");
    if (n_enc_layers < 1 || n_enc_layers > 16 || n_dec_layers < 1 || n_dec_layers > 16 || n_tokens < 1)
        return fail(B2H_ERR_UNSUPPORTED, "TextPoseTransformer: 1 <= n_enc_layers, n_dec_layers <= 16 and n_tokens >= 1");
    std::unique_ptr<b2h_tpt> m(new b2h_tpt()); // released to the caller only on success
    if (int rc = probe_device(m->device, m->num_cus)) return rc;
    if (int rc = set_tenc_kernel_attributes()) return rc;
    m->n_tokens = n_tokens;
    m->ninp = ninp;
    m->nout = nout;
    m->n_enc = n_enc_layers;
    m->n_dec = n_dec_layers;
    m->enc.resize(n_enc_layers);
    m->dec.resize(n_dec_layers);
    *out = m.release();
    return B2H_OK;
}

int b2h_tpt_destroy(b2h_tpt* m) {
    delete m;
    return B2H_OK;
}

int b2h_tpt_set_kernel(b2h_tpt* m, int kernel) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    if (kernel != B2H_TENC_F32 && kernel != B2H_TENC_F16X3) return fail(B2H_ERR_INVALID, "unknown TextPoseTransformer kernel");
    m->kernel = kernel;
    return B2H_OK;
}

int b2h_tpt_set_train_kernel(b2h_tpt* m, int kernel) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    if (kernel != B2H_TRAIN_VALU && kernel != B2H_TRAIN_MFMA) return fail(B2H_ERR_INVALID, "unknown TextPoseTransformer train kernel");
    m->train_kernel = kernel;
    return B2H_OK;
}

int b2h_tpt_set_train_linear(b2h_tpt* m, int kernel) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    if (kernel != B2H_TRAIN_VALU && kernel != B2H_TRAIN_MFMA) return fail(B2H_ERR_INVALID, "unknown TextPoseTransformer train Linear kernel");
    m->train_linear = kernel;
    return B2H_OK;
}

int b2h_tpt_set_train_whole(b2h_tpt* m, int kernel) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    if (kernel != B2H_TRAIN_VALU && kernel != B2H_TRAIN_MFMA) return fail(B2H_ERR_INVALID, "unknown TextPoseTransformer whole-matrix train kernel");
    m->train_whole = kernel;
    return B2H_OK;
}

int b2h_tpt_load_weights(b2h_tpt* m, const float* const* tensors, int count, int on_device) {
    if (!m || !tensors) return fail(B2H_ERR_INVALID, "NULL argument");
    if (count != 9 + 12 * m->n_enc + 18 * m->n_dec)
        return fail(B2H_ERR_INVALID, "expected 9 + 12*n_enc_layers + 18*n_dec_layers tensors");
    for (int i = 0; i < count; ++i)
        if (!tensors[i]) return fail(B2H_ERR_INVALID, "tensor pointer is NULL");
    const std::vector<size_t> sizes = tpt_param_floats(m);
    std::vector<std::vector<float>> h;
    int rc;
    if ((rc = fetch_tensors(tensors, sizes, on_device, h)) || (rc = check_device(m->device))) return rc;
    m->w_absmax = 0.f;
    for (int i = 0; i < count; ++i) m->w_absmax = absmax_of(h[i], m->w_absmax); // the table too: its rows are activations
    const int Di = kTencD;
    // one Linear of 128 inputs: rows [r0, r0 + 128) of tensor i with bias i + 1, and the LayerNorm that follows it
    const auto lin = [&](TencBlob& blob, int i, int r0, int norm) {
        return pack_blob(blob, h[i].data(), h[i + 1].data(), r0, Di, Di, norm >= 0 ? h[norm].data() : nullptr,
                         norm >= 0 ? h[norm + 1].data() : nullptr);
    };
    const auto heads = [&](TencBlob (&hb)[kTencHeads], int i) { return pack_qkv_heads(hb, h[i].data(), h[i + 1].data()); };
    const auto norm = [&](DevBuf& buf, int i) {
        std::vector<float> gb(h[i]);
        gb.insert(gb.end(), h[i + 1].begin(), h[i + 1].end());
        return buf.upload(gb.data(), gb.size() * 4);
    };
    for (int l = 0; l < m->n_enc; ++l) {
        auto& L = m->enc[l];
        const int o = 12 * l;
        if ((rc = lin(L.q, o, 0, -1)) || (rc = lin(L.k, o, Di, -1)) || (rc = lin(L.v, o, 2 * Di, -1)) ||
            (rc = lin(L.attn_out, o + 2, 0, o + 8)) || (rc = lin(L.ff1, o + 4, 0, -1)) || (rc = lin(L.ff2, o + 6, 0, o + 10)) ||
            (rc = heads(L.qkv_head, o)))
            return rc;
    }
    int o = 12 * m->n_enc;
    if ((rc = norm(m->enc_norm, o))) return rc;
    o += 2;
    for (int l = 0; l < m->n_dec; ++l, o += 18) {
        auto& L = m->dec[l];
        if ((rc = lin(L.q, o, 0, -1)) || (rc = lin(L.k, o, Di, -1)) || (rc = lin(L.v, o, 2 * Di, -1)) ||
            (rc = lin(L.attn_out, o + 2, 0, o + 12)) || (rc = lin(L.cq, o + 4, 0, -1)) || (rc = lin(L.ck, o + 4, Di, -1)) ||
            (rc = lin(L.cv, o + 4, 2 * Di, -1)) || (rc = lin(L.cross_out, o + 6, 0, o + 14)) ||
            (rc = lin(L.ff1, o + 8, 0, -1)) || (rc = lin(L.ff2, o + 10, 0, o + 16)) || (rc = heads(L.qkv_head, o)) ||
            (rc = heads(L.cross_head, o + 4)))
            return rc;
    }
    if ((rc = norm(m->dec_norm, o))) return rc;
    o += 2;
    if ((rc = m->table.upload(h[o].data(), h[o].size() * 4))) return rc;
    if ((rc = pack_blob(m->out_proj, h[o + 1].data(), h[o + 2].data(), 0, m->nout, Di, nullptr, nullptr, 0, kTptHeadMpad))) return rc;
    if ((rc = pack_blob(m->in_proj, h[o + 3].data(), h[o + 4].data(), 0, Di, m->ninp, nullptr, nullptr, tpt_front_kpad(m->ninp))))
        return rc;
    m->has_weights = true;
    return B2H_OK;
}

size_t b2h_tpt_workspace_bytes(const b2h_tpt* m, int64_t B, int64_t S, int64_t T) {
    if (!m || B < 0 || S < 0 || T < 0) return 0;
    const int64_t frame = kTptFrameFloats + (tpt_padded_rows(m) ? kTptPadLd : 0);
    return ((size_t)B * S * (kTptTokenFloats + kTptTokenLayerFloats * m->n_dec) + (size_t)B * T * frame) * sizeof(float);
}


// Both forwards.  max_frames is the caller's limit on T: 128 for b2h_tpt_forward, B2H_TPT_MAX_FRAMES for
// b2h_tpt_forward_fused.  T <= 128 runs the launches this model has always run, whatever the entry point; T > 128
// runs the decoder on row sets in both arithmetics -- the chains write Q | K | V, the cross query and the memory's
// K | V, as the fp32 path always did -- with b2h_attn_long_* for its two attentions (kernel_attn_long.h).
// text_len / frame_len: (B) key lengths or nullptr, the three key-padding masks of DESIGN.md section 33 (exact fp32
// only).
static int tpt_launch(b2h_tpt* m, const int64_t* tokens, const float* x, float* y, int64_t B, int64_t S, int64_t T,
                      const FusedArgs& fa, int64_t max_frames, const int64_t* text_len, const int64_t* frame_len,
                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    if (!m->has_weights) return fail(B2H_ERR_NO_WEIGHTS, "b2h_tpt_forward before b2h_tpt_load_weights");
    if (B < 0 || S < 1 || T < 1) return fail(B2H_ERR_SHAPE, "expected B >= 0, S >= 1 and T >= 1");
    if (S > kTptMaxLen || T > max_frames)
        return fail(B2H_ERR_SHAPE, max_frames > kTptMaxLen
                                       ? "TextPoseTransformer: S is limited to 128 and T to B2H_TPT_MAX_FRAMES = 1024"
                                       : "TextPoseTransformer: S and T are limited to 128 (the reference's datasets feed 40 "
                                         "tokens and 100 frames, text_pose_dataset.py:467-470); b2h_tpt_forward_fused "
                                         "takes T <= 1024");
    if (B == 0) return B2H_OK;
    if (!tokens || !x || !y || !workspace) return fail(B2H_ERR_INVALID, "NULL pointer");
    if (misaligned(tokens, 8) || misaligned(x, 16) || misaligned(y, 8) || misaligned(workspace, 16))
        return fail(B2H_ERR_INVALID, "x and workspace must be 16-byte aligned, tokens and y 8-byte aligned");
    if (workspace_bytes < b2h_tpt_workspace_bytes(m, B, S, T)) return fail(B2H_ERR_INVALID, "workspace too small");
    if (misaligned(text_len, 8) || misaligned(frame_len, 8))
        return fail(B2H_ERR_INVALID, "text_len and frame_len must be 8-byte aligned int64 arrays");
    for (const int64_t* len : {text_len, frame_len})
        if (len && (overlaps(len, (size_t)B * 8, y, (size_t)B * T * m->nout * 4) ||
                    overlaps(len, (size_t)B * 8, workspace, b2h_tpt_workspace_bytes(m, B, S, T))))
            return fail(B2H_ERR_INVALID, "y or the workspace overlaps a key length array");
    if (m->kernel == B2H_TENC_F16X3 && (text_len || frame_len))
        return fail(B2H_ERR_UNSUPPORTED, "B2H_TENC_F16X3 takes no key lengths (text_len / frame_len): its attention kernels "
                                         "attend to every row; select exact fp32 with b2h_tpt_set_kernel(fp32), i.e. "
                                         "b2h_tpt_set_kernel(m, B2H_TENC_F32)");
    const int64_t Ns = B * S, Nt = B * T;
    // grid limits: attention launches B x heads workgroups, the row kernels 8 rows per workgroup, the copy of
    // 42- / 58-float pose rows (b2h_item_pad_rows) 4 rows per workgroup
    if (B * kTencHeads > 0x7fffffff || std::max(Ns, Nt) / 8 >= 0x7fffffff || (tpt_padded_rows(m) && Nt / 4 >= 0x7fffffff))
        return fail(B2H_ERR_SHAPE, "batch too large for one launch");
    if (int rc = check_device(m->device)) return rc;
    if (m->kernel == B2H_TENC_F16X3 && !(m->w_absmax < kF16Max))
        return fail(B2H_ERR_UNSUPPORTED, "B2H_TENC_F16X3: a parameter is outside the f16 range (|w| >= 65504 or not "
                                         "finite); use B2H_TENC_F32");
    if (tpt_padded_rows(m) && (fa.flags & (kPreChest | kPreNorm)))
        return fail(B2H_ERR_INVALID, "B2H_PRE_CHEST_DIFF / B2H_PRE_NORMALIZE apply to body-only rows (ninp 16 or 24); the "
                                     "composite rows of ninp 42 / 58 are transformed by b2h_tpt_build_item");
    hipStream_t st = (hipStream_t)stream;
    const TptWs ws = tpt_ws(workspace, Ns, Nt, m->n_dec);
    const int nk = (int)((S + 15) / 16), nq = (int)((T + 15) / 16);
    // the rows pose2hidden_projection reads: x itself, or its zero-padded copy
    const float* xf = x;
    if (tpt_padded_rows(m)) {
        hipLaunchKernelGGL(b2h_item_pad_rows, dim3((unsigned)((Nt * kTptPadLd + 255) / 256)), dim3(256), 0, st, x, ws.XP, Nt, m->ninp);
        xf = ws.XP;
    }
    const int ldf = tpt_front_ld(m);
    const bool h3 = m->kernel == B2H_TENC_F16X3, long_t = T > kTptMaxLen;
    // the item transforms: on the pose rows as they enter pose2hidden_projection, in hidden2pose_projection's store
    const auto pre = [&](Chain& c) { c.a.flags = fa.flags & (kPreChest | kPreNorm); c.a.factor = fa.factor; };
    const auto post = [&](Chain& c) {
        c.a.flags = fa.flags & (kPostDenorm | kPostMask); c.a.factor = fa.factor; c.a.n_frames = fa.n_frames; c.a.Tseq = (int)T;
    };

    // encoder (torch.nn.TransformerEncoder, post-norm, ReLU): token_embedding -> layers -> encoder.norm
    hipLaunchKernelGGL(b2h_tpt_embed, dim3((unsigned)((Ns * 32 + 255) / 256)), dim3(256), 0, st, tokens,
                       (const float*)m->table.p, ws.MEM, Ns, m->n_tokens);
    if (h3) {
        // 4 + 2 n_enc + 4 n_dec launches: the attention kernels project Q, K, V themselves, so the chains carry no
        // Q, K, V stages and QKVs, MKV, QC and QKVt stay untouched (T <= 128; beyond, the decoder is the one below)
        for (int l = 0; l < m->n_enc; ++l) {
            const EncLayer& L = m->enc[l];
            self_attn_h3(L.qkv_head, ws.MEM, ws.OCs, B, (int)S, m->num_cus, st);
            Chain c = tpt_rows(ws.OCs, kTencD, ws.MEM, Ns, true);
            c.add_layer_tail(L.attn_out, L.ff1, L.ff2, ws.MEM, nullptr, nullptr);
            c.launch(m->num_cus, st);
        }
        tpt_layernorm(m->enc_norm, ws.MEM, Ns, st);
    }
    if (h3 && !long_t) {
        {
            Chain c = tpt_rows(xf, ldf, nullptr, Nt, true);
            pre(c);
            c.add(m->in_proj, ST_SET, ws.XT);
            c.launch(m->num_cus, st);
        }
        for (int l = 0; l < m->n_dec; ++l) {
            const auto& L = m->dec[l];
            self_attn_h3(L.qkv_head, ws.XT, ws.OCt, B, (int)T, m->num_cus, st);
            {   // self out_proj + x -> norm1 -> X1: one stage, whose result is copied out
                Chain c = tpt_rows(ws.OCt, kTencD, ws.XT, Nt, true);
                c.add(L.attn_out, ST_RESLN_GLOBAL, ws.X1);
                c.launch(m->num_cus, st);
            }
            AttnCrossArgs xa{};
            xa.x = ws.X1; xa.mem = ws.MEM; xa.out = ws.OCt; xa.T = (int)T; xa.S = (int)S; xa.B = B;
            for (int hd = 0; hd < kTencHeads; ++hd) xa.blob[hd] = (const float*)L.cross_head[hd].buf16.p;
            hipLaunchKernelGGL(kAttnCrossH3[nk - 1], dim3(attn_h3_grid(m->num_cus)), dim3(64 * nq),
                               (size_t)attn_qkv_lds_bytes(nk), st, xa);
            // cross out_proj + X1 -> norm2 -> linear1 ReLU -> linear2 + res -> norm3 -> XT
            Chain c = tpt_rows(ws.OCt, kTencD, ws.X1, Nt, true);
            c.add_layer_tail(L.cross_out, L.ff1, L.ff2, ws.XT, nullptr, nullptr);
            c.launch(m->num_cus, st);
        }
        tpt_layernorm(m->dec_norm, ws.XT, Nt, st);
        {
            Chain c = tpt_rows(ws.XT, kTencD, nullptr, Nt, true);
            post(c);
            c.add(m->out_proj, ST_STORE, y, m->nout);
            c.launch(m->num_cus, st);
        }
        HIP_TRY(hipGetLastError());
        return B2H_OK;
    }
    const auto qkv = [](Chain& c, const EncLayer& L, float* QKV) { c.add_qkv(L.q, L.k, L.v, QKV); };
    if (!h3) {
        {
            Chain c = tpt_rows(ws.MEM, kTencD, nullptr, Ns);
            qkv(c, m->enc[0], ws.QKVs);
            c.launch(m->num_cus, st);
        }
        for (int l = 0; l < m->n_enc; ++l) {
            const EncLayer& L = m->enc[l];
            attn_rows(st, false, self_src(ws.QKVs), ws.OCs, B, (int)S, (int)S, text_len);
            Chain c = tpt_rows(ws.OCs, kTencD, ws.MEM, Ns);
            c.add_layer_tail(L.attn_out, L.ff1, L.ff2, ws.MEM, l + 1 < m->n_enc ? &m->enc[l + 1] : nullptr, ws.QKVs);
            c.launch(m->num_cus, st);
        }
        tpt_layernorm(m->enc_norm, ws.MEM, Ns, st);
    }
    // The decoder on row sets: fp32 at any T, f16x3 at T > 128 (h3 chains, b2h_attn_long_h3).
    // K and V of the memory for every decoder layer: two ST_STORE stages per layer, four layers per launch
    for (int l0 = 0; l0 < m->n_dec; l0 += kChainMaxStages / 2) {
        Chain c = tpt_rows(ws.MEM, kTencD, nullptr, Ns, h3);
        for (int l = l0; l < std::min(m->n_dec, l0 + kChainMaxStages / 2); ++l) {
            float* kv = ws.MKV + (int64_t)l * Ns * kTptTokenLayerFloats;
            c.add(m->dec[l].ck, ST_STORE, kv, 2 * kTencD);
            c.add(m->dec[l].cv, ST_STORE, kv + kTencD, 2 * kTencD);
        }
        c.launch(m->num_cus, st);
    }

    // decoder (torch.nn.TransformerDecoder): pose2hidden_projection -> layers -> decoder.norm -> hidden2pose_projection
    {
        Chain c = tpt_rows(xf, ldf, nullptr, Nt, h3);
        pre(c);
        c.add(m->in_proj, ST_SET, ws.XT);
        qkv(c, m->dec[0], ws.QKVt);
        c.launch(m->num_cus, st);
    }
    for (int l = 0; l < m->n_dec; ++l) {
        const auto& L = m->dec[l];
        attn_rows(st, h3, self_src(ws.QKVt), ws.OCt, B, (int)T, (int)T, frame_len);
        {   // self out_proj + x -> norm1 -> X1; the cross-attention query of X1
            Chain c = tpt_rows(ws.OCt, kTencD, ws.XT, Nt, h3);
            c.add(L.attn_out, ST_RESLN_GLOBAL, ws.X1);
            c.add(L.cq, ST_STORE, ws.QC);
            c.launch(m->num_cus, st);
        }
        // S <= 128: one key block at any T
        attn_rows(st, h3, cross_src(ws.QC, ws.MKV + (int64_t)l * Ns * kTptTokenLayerFloats), ws.OCt, B, (int)T, (int)S,
                  text_len);
        // cross out_proj + X1 -> norm2 -> linear1 ReLU -> linear2 + res -> norm3 -> XT [+ the next layer's Q, K, V]
        Chain c = tpt_rows(ws.OCt, kTencD, ws.X1, Nt, h3);
        c.add_layer_tail(L.cross_out, L.ff1, L.ff2, ws.XT, l + 1 < m->n_dec ? &m->dec[l + 1] : nullptr, ws.QKVt);
        c.launch(m->num_cus, st);
    }
    tpt_layernorm(m->dec_norm, ws.XT, Nt, st);
    {
        Chain c = tpt_rows(ws.XT, kTencD, nullptr, Nt, h3);
        post(c);
        c.add(m->out_proj, ST_STORE, y, m->nout);
        c.launch(m->num_cus, st);
    }
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

int b2h_tpt_forward(b2h_tpt* m, const int64_t* tokens, const float* x, float* y, int64_t B, int64_t S, int64_t T,
                    void* workspace, size_t workspace_bytes, void* stream) {
    const FusedArgs fa{0, 1.0f, nullptr};
    return tpt_launch(m, tokens, x, y, B, S, T, fa, kTptMaxLen, nullptr, nullptr, workspace, workspace_bytes, stream);
}

int b2h_tpt_forward_masked(b2h_tpt* m, const int64_t* tokens, const float* body, float* y, int64_t B, int64_t S, int64_t T,
                           int flags, float factor, const int64_t* n_frames, const int64_t* text_len,
                           const int64_t* frame_len, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_fused(flags, factor)) return rc;
    if ((flags & kPostMask) && !n_frames) return fail(B2H_ERR_INVALID, "B2H_POST_MASK_TAIL needs n_frames");
    const FusedArgs fa{flags, factor, n_frames};
    return tpt_launch(m, tokens, body, y, B, S, T, fa, B2H_TPT_MAX_FRAMES, text_len, frame_len, workspace, workspace_bytes,
                      stream);
}

int b2h_tpt_forward_fused(b2h_tpt* m, const int64_t* tokens, const float* body, float* y, int64_t B, int64_t S, int64_t T,
                          int flags, float factor, const int64_t* n_frames, void* workspace, size_t workspace_bytes,
                          void* stream) {
    return b2h_tpt_forward_masked(m, tokens, body, y, B, S, T, flags, factor, n_frames, nullptr, nullptr, workspace,
                                  workspace_bytes, stream);
}

int b2h_token_lengths(const int64_t* tokens, int64_t B, int64_t S, int64_t pad_id, int64_t* lengths, void* stream) {
    if (B < 0 || S < 1) return fail(B2H_ERR_SHAPE, "b2h_token_lengths: expected B >= 0 and S >= 1");
    if (S > 0x7fffffff || (B + 3) / 4 > 0x7fffffff) return fail(B2H_ERR_SHAPE, "b2h_token_lengths: batch too large for one launch");
    if (B == 0) return B2H_OK;
    if (!tokens || !lengths) return fail(B2H_ERR_INVALID, "b2h_token_lengths: tokens / lengths is NULL");
    if (misaligned(tokens, 8) || misaligned(lengths, 8))
        return fail(B2H_ERR_INVALID, "b2h_token_lengths: tokens and lengths must be 8-byte aligned");
    if (int rc = check_overlap({{lengths, (size_t)B * 8}}, {{tokens, (size_t)B * S * 8, "tokens"}})) return rc;
    hipLaunchKernelGGL(b2h_token_lengths_k, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, tokens, B, (int)S,
                       pad_id, lengths);
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

int b2h_tpt_info(const b2h_tpt* m, int* n_tokens, int* ninp, int* nout, int* n_enc_layers, int* n_dec_layers,
                 int* has_weights) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    if (n_tokens) *n_tokens = m->n_tokens;
    if (ninp) *ninp = m->ninp;
    if (nout) *nout = m->nout;
    if (n_enc_layers) *n_enc_layers = m->n_enc;
    if (n_dec_layers) *n_dec_layers = m->n_dec;
    if (has_weights) *has_weights = m->has_weights ? 1 : 0;
    return B2H_OK;
}

int b2h_tpt_build_item(const float* body, const float* right_hand, float* item, int64_t B, int64_t T, int predict,
                       int flags, float factor, void* stream) {
    if (B < 0 || T < 0) return fail(B2H_ERR_SHAPE, "negative shape");
    if (predict != B2H_PREDICT_RIGHT_INDEX && predict != B2H_PREDICT_RIGHT_3FINGERS)
        return fail(B2H_ERR_INVALID, "predict must be B2H_PREDICT_RIGHT_INDEX or B2H_PREDICT_RIGHT_3FINGERS");
    if (flags & ~(kPreChest | kPreNorm)) return fail(B2H_ERR_INVALID, "unknown flag bits (only B2H_PRE_* apply)");
    if ((flags & kPreNorm) && !(factor > 0.f)) return fail(B2H_ERR_INVALID, "factor must be > 0");
    if (B * T == 0) return B2H_OK;
    if (B > 0x7fffffff || T > (1 << 24)) return fail(B2H_ERR_SHAPE, "shape too large");
    int rc;
    if ((rc = check_device_ptr(body, "body")) || (rc = check_device_ptr(right_hand, "right_hand")) ||
        (rc = check_device_ptr(item, "item")))
        return rc;
    if (misaligned(body, 8) || misaligned(right_hand, 8) || misaligned(item, 8))
        return fail(B2H_ERR_INVALID, "body, right_hand and item must be 8-byte aligned");
    const int nj = predict == B2H_PREDICT_RIGHT_INDEX ? 29 : 21;
    const size_t in = (size_t)B * T * nj * 8;
    if (overlaps(item, in, body, (size_t)B * T * kInCh * 4) || overlaps(item, in, right_hand, (size_t)B * T * kOutCh * 4))
        return fail(B2H_ERR_INVALID, "item overlaps an input");
    const int64_t n = B * T * nj;
    if ((n + 255) / 256 > 0x7fffffff) return fail(B2H_ERR_SHAPE, "shape too large");
    hipLaunchKernelGGL(b2h_item_build_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, body,
                       right_hand, item, B * T, predict, flags, factor);
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

} // extern "C"

// ---- TransformerEnc training (kernel_tenc_train.h) ------------------------------------------------------------
namespace {

constexpr int64_t kTtSavedFrame = kInCh + kTtD;                  // X0, H0: floats per frame
constexpr int64_t kTtSavedLayer = 3 * kTtD + 6 * kTtD + 4;       // QKV, O, R1, H1, F1, R2, H2, {mean, rstd} x 2
constexpr int64_t kTtScratchFrame = 4 * kTtD + 3 * kTtD;         // gA, gB, gBm, gC, gQ
constexpr int64_t kTtSlab = (int64_t)3 * kTtD * kTtD + 3 * kTtD; // the largest Linear: in_proj weight + bias

// Saved activations of one layer (floats, N = B * T rows each).
struct TtLayer {
    float *QKV, *O, *R1, *H1, *F1, *R2, *H2, *ST;
};
TtLayer tt_layer(float* layers, int64_t N, int l) { // layers: where layer 0 starts
    float* p = layers + (int64_t)l * N * kTtSavedLayer;
    return TtLayer{p, p + N * 384, p + N * 512, p + N * 640, p + N * 768, p + N * 896, p + N * 1024, p + N * 1152};
}

size_t tt_saved_bytes(int nlayers, int64_t N) { return (size_t)N * (kTtSavedFrame + nlayers * kTtSavedLayer) * 4; }
size_t tt_scratch_bytes(int64_t N) { return ((size_t)N * kTtScratchFrame + (size_t)tt_nslabs(N) * kTtSlab) * 4; }

// Why the training calls refuse a (B, T) batch, or nullptr (b2h_tenc_mask_numel answers the same shapes).
const char* tt_shape_refusal(const b2h_tenc* m, int64_t B, int64_t T) {
    if (B < 0 || T < 1) return "expected B >= 0 and T >= 1";
    if (T > m->max_len || T > 128)
        return "TransformerEnc: T exceeds the positional encoding's max_len (src + pe[:T], HandPoseModels.py:101,167)";
    // grid limits: attention launches B x heads workgroups, LayerNorm N / 4 (the largest row grid), the Linears N / 16
    if (B * kTtHeads > 0x7fffffff || B * T / 4 >= 0x7fffffff) return "batch too large for one launch";
    return nullptr;
}

int tenc_nmasks(const b2h_tenc* m) { return 1 + 4 * m->nlayers; }

// Elements of every keep-mask, in the order of `masks`: pos, then per layer attn, drop1, ff, drop2.
std::vector<size_t> tenc_mask_bytes(const b2h_tenc* m, int64_t B, int64_t T) {
    std::vector<size_t> n(tenc_nmasks(m), (size_t)B * T * kTtD);
    n[0] = (size_t)B * T * kInCh;
    for (size_t i = 1; i < n.size(); i += 4) n[i] = (size_t)B * kTtHeads * T * T;
    return n;
}

// Checks shared by the train_forward and backward of both transformers (the model is not NULL), as tenc_launch makes
// them.  shape_refusal: why the model refuses the batch, or nullptr.
int tt_check(const char* shape_refusal, const float* const* params, size_t nparams, const uint8_t* const* masks, int nmasks,
             float p) {
    if (!params) return fail(B2H_ERR_INVALID, "params is NULL");
    if (!(p >= 0.f && p <= 1.f)) return fail(B2H_ERR_INVALID, "dropout p must be in [0, 1]");
    if ((p > 0.f) != (masks != nullptr)) return fail(B2H_ERR_INVALID, "masks must be given exactly when p > 0");
    if (shape_refusal) return fail(B2H_ERR_SHAPE, shape_refusal);
    for (size_t i = 0; i < nparams; ++i) {
        if (!params[i]) return fail(B2H_ERR_INVALID, "params[" + std::to_string(i) + "] is NULL");
        if (misaligned(params[i], 4)) return fail(B2H_ERR_INVALID, "params must be 4-byte aligned fp32 tensors");
    }
    if (masks)
        for (int i = 0; i < nmasks; ++i)
            if (!masks[i]) return fail(B2H_ERR_INVALID, "masks[" + std::to_string(i) + "] is NULL");
    return B2H_OK;
}

// The read-only operands of a training call for check_overlap: its plain inputs, the parameters (floats each) and
// the masks (bytes each).
std::vector<Span> tt_read_only(const float* const* params, const std::vector<size_t>& floats, const uint8_t* const* masks,
                               const std::vector<size_t>& mask_bytes, std::vector<Span> ins) {
    ins.reserve(ins.size() + floats.size() + mask_bytes.size());
    for (Span& in : ins) in.what = "an input";
    for (size_t i = 0; i < floats.size(); ++i) ins.push_back({params[i], floats[i] * 4, "a parameter"});
    if (masks)
        for (size_t i = 0; i < mask_bytes.size(); ++i) ins.push_back({masks[i], mask_bytes[i], "a mask"});
    return ins;
}

unsigned tt_row_blocks(int64_t N, int rows) { return (unsigned)((N + rows - 1) / rows); }

// Where a training call runs and which Linear trio it launches: kernel_tenc_train.h's on the vector ALU, or
// kernel_train_linear_mfma.h's on the matrix cores (after b2h_tpt_set_train_linear / b2h_tenc_set_train_linear only).
struct TtLin {
    hipStream_t st;
    bool mfma;
};

void tt_linear(const TtLin& ln, const float* X, const float* W, const float* b, float* Y, int64_t N, int K, int M,
               int relu, const uint8_t* mask, float scale, const float* res) {
    hipStream_t st = ln.st;
    if (ln.mfma) {
        hipLaunchKernelGGL(b2h_ml_linear, dim3(tt_row_blocks(N, kMlRows)), dim3(256), kMlFwdLds, st, X, W, b, Y, N, K, M, relu,
                           mask, scale, res);
        return;
    }
    hipLaunchKernelGGL(b2h_tt_linear, dim3(tt_row_blocks(N, kTtRows)), dim3(128), 0, st, X, W, b, Y, N, K, M, relu, mask,
                       scale, res);
}

void tt_linear_dx(const TtLin& ln, const float* dY, const float* W, float* dX, int64_t N, int K, int M, const float* gate,
                  const uint8_t* mask, float scale, const float* add) {
    hipStream_t st = ln.st;
    if (ln.mfma) {
        hipLaunchKernelGGL(b2h_ml_linear_dx, dim3(tt_row_blocks(N, kMlRows)), dim3(256), kMlDxLds, st, dY, W, dX, N, K, M, gate,
                           mask, scale, add);
        return;
    }
    hipLaunchKernelGGL(b2h_tt_linear_dx, dim3(tt_row_blocks(N, kTtRows)), dim3(128), 0, st, dY, W, dX, N, K, M, gate,
                       mask, scale, add);
}

// dW, db of one Linear: slab partials, then the fixed-order sum into the gradient tensors.
void tt_linear_dw(const TtLin& ln, const float* dY, const float* X, float* slabs, int64_t N, int K, int M, float* gW,
                  float* gb) {
    hipStream_t st = ln.st;
    const int S = tt_nslabs(N);
    const dim3 grid(S, (M + kTtDwM - 1) / kTtDwM);
    if (ln.mfma)
        hipLaunchKernelGGL(b2h_ml_linear_dw, grid, dim3(256), kMlDwLds, st, dY, X, slabs, kTtSlab, N, K, M);
    else
        hipLaunchKernelGGL(b2h_tt_linear_dw, grid, dim3(256), 0, st, dY, X, slabs, kTtSlab, N, K, M);
    hipLaunchKernelGGL(b2h_tt_reduce, dim3((M * K + M + 255) / 256), dim3(256), 0, st, slabs, kTtSlab, S, gW, M * K, gb, M);
}

void tt_layernorm_bwd(hipStream_t st, const float* dY, const float* X, const float* stats, const float* gamma, float* dX,
                      float* dXm, const uint8_t* mask, float scale, float* slabs, int64_t N, float* ggamma, float* gbeta) {
    const int S = tt_nslabs(N);
    hipLaunchKernelGGL(b2h_tt_layernorm_bwd, dim3(S), dim3(256), 0, st, dY, X, stats, 4, gamma, dX, dXm, mask, scale,
                       slabs, kTtSlab, N);
    hipLaunchKernelGGL(b2h_tt_reduce, dim3(1), dim3(256), 0, st, slabs, kTtSlab, S, ggamma, kTtD, gbeta, kTtD);
}

float tt_scale(float p) { return p < 1.f ? 1.f / (1.f - p) : 0.f; }

// Which kernels run an attention in training: a whole-matrix pair up to 128 x 128, on the vector ALU
// (kernel_train_attn.h) or on the matrix cores (kernel_train_attn_whole_mfma.h); beyond that the blocked ones, on the
// vector ALU (kernel_train_attn_long.h) or on the matrix cores (kernel_train_attn_mfma.h).
enum class TrainAttn { kWhole, kBlockedValu, kBlockedMfma, kWholeMfma };

// The gradients of self-attention over [Q | K | V] rows (N, 384): [dQ | dK | dV] in the same layout (self_src's counterpart).
LtGradDst self_dst(float* gQ) { return LtGradDst{gQ, 3 * kTtD, 0, gQ, 3 * kTtD, kTtD, 2 * kTtD}; }

// Attention of B sequences of Tq query rows over Tk key rows in training: O (B*Tq, 128) and, from the blocked kernels
// only, the rows' log-sum-exp (B, 4, Tq).
// klen: (B) key lengths or nullptr (tt_key_len).
void train_sdpa(hipStream_t st, TrainAttn route, const AttnSrc& src, const uint8_t* mask, float sc, float* O, float* lse,
                int64_t B, int Tq, int Tk, const int64_t* klen) {
    const unsigned heads = (unsigned)(B * kTtHeads);
    const dim3 grid(heads, lt_blocks(Tq, kLtQb));
    if (route == TrainAttn::kWhole)
        hipLaunchKernelGGL(b2h_tt_sdpa, dim3(heads), dim3(256), tt_sdpa_lds_bytes(Tq, Tk, false), st, src, mask, sc, O, Tq, Tk,
                           klen);
    else if (route == TrainAttn::kWholeMfma)
        hipLaunchKernelGGL(b2h_mw_sdpa, dim3(heads), dim3(256), mw_sdpa_lds_bytes(Tq, Tk, false), st, src, mask, sc, O, Tq, Tk,
                           klen);
    else if (route == TrainAttn::kBlockedMfma)
        hipLaunchKernelGGL(b2h_mt_sdpa, grid, dim3(256), kMtFwdLds, st, src, mask, sc, O, lse, Tq, Tk, klen);
    else
        hipLaunchKernelGGL(b2h_lt_sdpa, grid, dim3(256), kLtFwdLds, st, src, mask, sc, O, lse, Tq, Tk, klen);
}

// Its backward.  Blocked: the query owner (dQ, and the row terms D for the key owner), then the key owner (dK, dV).
void train_sdpa_bwd(hipStream_t st, TrainAttn route, const AttnSrc& src, const float* dO, const float* lse, float* D,
                    const uint8_t* mask, float sc, const LtGradDst& dst, int64_t B, int Tq, int Tk, const int64_t* klen) {
    const unsigned heads = (unsigned)(B * kTtHeads);
    const dim3 gq(heads, lt_blocks(Tq, kLtQb)), gkv(heads, lt_blocks(Tk, kLtKb));
    if (route == TrainAttn::kWhole) {
        hipLaunchKernelGGL(b2h_tt_sdpa_bwd, dim3(heads), dim3(256), tt_sdpa_lds_bytes(Tq, Tk, true), st, src, dO, mask, sc, dst,
                           Tq, Tk, klen);
    } else if (route == TrainAttn::kWholeMfma) {
        hipLaunchKernelGGL(b2h_mw_sdpa_bwd, dim3(heads), dim3(256), mw_sdpa_lds_bytes(Tq, Tk, true), st, src, dO, mask, sc, dst,
                           Tq, Tk, klen);
    } else if (route == TrainAttn::kBlockedMfma) {
        hipLaunchKernelGGL(b2h_mt_sdpa_bwd_q, gq, dim3(256), kMtBwdQLds, st, src, dO, lse, D, mask, sc, dst, Tq, Tk, klen);
        hipLaunchKernelGGL(b2h_mt_sdpa_bwd_kv, gkv, dim3(256), kMtBwdKvLds, st, src, dO, lse, D, mask, sc, dst, Tq, Tk, klen);
    } else {
        hipLaunchKernelGGL(b2h_lt_sdpa_bwd_q, gq, dim3(256), kLtBwdQLds, st, src, dO, lse, D, mask, sc, dst, Tq, Tk, klen);
        hipLaunchKernelGGL(b2h_lt_sdpa_bwd_kv, gkv, dim3(256), kLtBwdKvLds, st, src, dO, lse, D, mask, sc, dst, Tq, Tk, klen);
    }
}

// One torch.nn.TransformerEncoderLayer (post-norm, ReLU) over N = B * T rows in training mode: H -> L.H2.
// w: its twelve tensors in state_dict order; mk: its four keep-masks attn, drop1, ff, drop2, or nullptr; attn: one of
// the two whole-matrix routes (T <= 128); klen: (B) key lengths or nullptr.
void tt_enc_layer_forward(const TtLin& ln, TrainAttn attn, const float* const* w, const TtLayer& L, const float* H,
                          int64_t B, int T, const uint8_t* const* mk, float sc, const int64_t* klen) {
    hipStream_t st = ln.st;
    const int64_t N = B * T;
    const auto mask = [&](int i) { return mk ? mk[i] : nullptr; };
    tt_linear(ln, H, w[0], w[1], L.QKV, N, kTtD, 3 * kTtD, 0, nullptr, 1.f, nullptr);
    train_sdpa(st, attn, self_src(L.QKV), mask(0), sc, L.O, nullptr, B, T, T, klen);
    tt_linear(ln, L.O, w[2], w[3], L.R1, N, kTtD, kTtD, 0, mask(1), sc, H);
    hipLaunchKernelGGL(b2h_tt_layernorm, dim3(tt_row_blocks(N, 4)), dim3(256), 0, st, L.R1, w[8], w[9], L.H1, L.ST, 4, N);
    tt_linear(ln, L.H1, w[4], w[5], L.F1, N, kTtD, kTtD, 1, mask(2), sc, nullptr);
    tt_linear(ln, L.F1, w[6], w[7], L.R2, N, kTtD, kTtD, 0, mask(3), sc, L.H1);
    hipLaunchKernelGGL(b2h_tt_layernorm, dim3(tt_row_blocks(N, 4)), dim3(256), 0, st, L.R2, w[10], w[11], L.H2, L.ST + 2, 4, N);
}

// The gradient rows of a backward pass (N rows each): four 128-wide, one 384-wide, then the slabs.
struct TtGrad {
    float *gA, *gB, *gBm, *gC, *gQ, *slabs;
};
TtGrad tt_grad(float* scratch, int64_t N) {
    return TtGrad{scratch, scratch + N * kTtD, scratch + N * 2 * kTtD, scratch + N * 3 * kTtD, scratch + N * 4 * kTtD,
                  scratch + N * kTtScratchFrame};
}

// Backward of tt_enc_layer_forward: G.gA = dH2 on entry, = dH_in on return; g: the layer's twelve gradients.
void tt_enc_layer_backward(const TtLin& ln, TrainAttn attn, const float* const* w, float* const* g, const TtLayer& L,
                           const float* Hin, const TtGrad& G, int64_t B, int T, const uint8_t* const* mk, float sc,
                           const int64_t* klen) {
    hipStream_t st = ln.st;
    const int64_t N = B * T;
    const auto mask = [&](int i) { return mk ? mk[i] : nullptr; };
    // norm2: gA = dH2 -> gB = dR2 (also dH1 through the residual), gBm = dR2 through drop2
    tt_layernorm_bwd(st, G.gA, L.R2, L.ST + 2, w[10], G.gB, G.gBm, mask(3), sc, G.slabs, N, g[10], g[11]);
    const float* dF = mk ? G.gBm : G.gB;
    tt_linear_dw(ln, dF, L.F1, G.slabs, N, kTtD, kTtD, g[6], g[7]);
    tt_linear_dx(ln, dF, w[6], G.gC, N, kTtD, kTtD, L.F1, nullptr, mk ? sc : 1.f, nullptr); // through drop_ff and ReLU
    tt_linear_dw(ln, G.gC, L.H1, G.slabs, N, kTtD, kTtD, g[4], g[5]);
    tt_linear_dx(ln, G.gC, w[4], G.gA, N, kTtD, kTtD, nullptr, nullptr, 1.f, G.gB);              // gA = dH1
    // norm1: gA -> gB = dR1 (also dH_in through the residual), gBm through drop1
    tt_layernorm_bwd(st, G.gA, L.R1, L.ST, w[8], G.gB, G.gBm, mask(1), sc, G.slabs, N, g[8], g[9]);
    const float* dA = mk ? G.gBm : G.gB;
    tt_linear_dw(ln, dA, L.O, G.slabs, N, kTtD, kTtD, g[2], g[3]);
    tt_linear_dx(ln, dA, w[2], G.gC, N, kTtD, kTtD, nullptr, nullptr, 1.f, nullptr);             // gC = dO
    train_sdpa_bwd(st, attn, self_src(L.QKV), G.gC, nullptr, nullptr, mask(0), sc, self_dst(G.gQ), B, T, T, klen);
    tt_linear_dw(ln, G.gQ, Hin, G.slabs, N, kTtD, 3 * kTtD, g[0], g[1]);
    tt_linear_dx(ln, G.gQ, w[0], G.gA, N, kTtD, 3 * kTtD, nullptr, nullptr, 1.f, G.gB);          // gA = dH_in
}

// Which attention pair and which Linear trio TransformerEnc's training calls launch, as b2h_tenc_set_train_kernel and
// b2h_tenc_set_train_linear chose, at every (B, T): the one place each that decides; the dispatch and the name
// functions both ask it.
TrainAttn tenc_train_attn(const b2h_tenc* m) {
    return m->train_kernel == B2H_TRAIN_MFMA ? TrainAttn::kWholeMfma : TrainAttn::kWhole;
}
bool tenc_train_linear_mfma(const b2h_tenc* m) { return m->train_linear == B2H_TRAIN_MFMA; }

} // namespace

extern "C" {

int b2h_tenc_set_train_kernel(b2h_tenc* m, int kernel) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    if (kernel != B2H_TRAIN_VALU && kernel != B2H_TRAIN_MFMA) return fail(B2H_ERR_INVALID, "unknown training kernel");
    m->train_kernel = kernel;
    return B2H_OK;
}

int b2h_tenc_set_train_linear(b2h_tenc* m, int kernel) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    if (kernel != B2H_TRAIN_VALU && kernel != B2H_TRAIN_MFMA) return fail(B2H_ERR_INVALID, "unknown training kernel");
    m->train_linear = kernel;
    return B2H_OK;
}

const char* b2h_tenc_train_attn_name(const b2h_tenc* m, int64_t T) {
    if (!m || tt_shape_refusal(m, 1, T)) return nullptr;
    return tenc_train_attn(m) == TrainAttn::kWholeMfma ? "b2h_mw_sdpa" : "b2h_tt_sdpa";
}

const char* b2h_tenc_train_linear_name(const b2h_tenc* m) {
    if (!m) return nullptr;
    return tenc_train_linear_mfma(m) ? "b2h_ml_linear" : "b2h_tt_linear";
}

size_t b2h_tenc_train_bytes(const b2h_tenc* m, int64_t B, int64_t T, int which) {
    if (!m || B < 1 || T < 1 || (which != 0 && which != 1)) return 0;
    return which == 0 ? tt_saved_bytes(m->nlayers, B * T) : tt_scratch_bytes(B * T);
}

int b2h_tenc_train_forward(b2h_tenc* m, const float* const* params, const float* x, const uint8_t* const* masks, float p,
                           float* y, void* saved, size_t saved_bytes, int64_t B, int64_t T, void* stream) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    if (int rc = tt_check(tt_shape_refusal(m, B, T), params, m->sizes.size(), masks, tenc_nmasks(m), p)) return rc;
    if (B == 0) return B2H_OK;
    if (!x || !y || !saved) return fail(B2H_ERR_INVALID, "NULL pointer");
    if (int rc = check_device(m->device)) return rc;
    if (misaligned(x, 16) || misaligned(y, 16) || misaligned(saved, 16))
        return fail(B2H_ERR_INVALID, "x, y and the saved buffer must be 16-byte aligned");
    const int64_t N = B * T;
    const size_t need = tt_saved_bytes(m->nlayers, N);
    if (saved_bytes < need)
        return fail(B2H_ERR_INVALID, "saved buffer smaller than b2h_tenc_train_bytes (" + std::to_string(need) + " B)");
    if (int rc = check_overlap({{y, (size_t)N * kOutCh * 4}, {saved, need}},
                               tt_read_only(params, m->sizes, masks, tenc_mask_bytes(m, B, T), {{x, (size_t)N * kInCh * 4}})))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const TtLin ln{st, tenc_train_linear_mfma(m)};
    const TrainAttn attn = tenc_train_attn(m);
    const float sc = tt_scale(p);
    auto mk = [&](int i) { return masks ? masks[i] : nullptr; };
    float* S = static_cast<float*>(saved);
    float* X0 = S;
    float* H = S + N * kInCh;
    float* Ls = S + N * kTtSavedFrame;
    hipLaunchKernelGGL(b2h_tt_posenc, dim3((unsigned)std::min<int64_t>((N * kInCh + 255) / 256, 4096)), dim3(256), 0, st, x,
                       params[0], mk(0), sc, X0, N, (int)T);
    tt_linear(ln, X0, params[1], params[2], H, N, kInCh, kTtD, 0, nullptr, 1.f, nullptr);
    for (int l = 0; l < m->nlayers; ++l) {
        const TtLayer L = tt_layer(Ls, N, l);
        tt_enc_layer_forward(ln, attn, params + 3 + 12 * l, L, H, B, (int)T, masks ? masks + 1 + 4 * l : nullptr, sc, nullptr);
        H = L.H2;
    }
    const float* const* wh = params + 3 + 12 * m->nlayers;
    tt_linear(ln, H, wh[0], wh[1], y, N, kTtD, kOutCh, 0, nullptr, 1.f, nullptr);
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

int b2h_tenc_backward(b2h_tenc* m, const float* const* params, const uint8_t* const* masks, float p, const float* dy,
                      const void* saved, size_t saved_bytes, float* dx, float* const* grads, void* scratch,
                      size_t scratch_bytes, int64_t B, int64_t T, void* stream) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    if (int rc = tt_check(tt_shape_refusal(m, B, T), params, m->sizes.size(), masks, tenc_nmasks(m), p)) return rc;
    if (B == 0) return fail(B2H_ERR_SHAPE, "b2h_tenc_backward needs B >= 1 (the gradients of an empty batch are not defined here)");
    if (!dy || !saved || !scratch) return fail(B2H_ERR_INVALID, "dy / saved / scratch is NULL");
    if (!grads) return fail(B2H_ERR_INVALID, "grads is NULL");
    if (int rc = check_device(m->device)) return rc;
    if (misaligned(dy, 16) || misaligned(saved, 16) || misaligned(scratch, 16) || (dx && misaligned(dx, 16)))
        return fail(B2H_ERR_INVALID, "dy, dx, the saved buffer and the scratch must be 16-byte aligned");
    const int64_t N = B * T;
    const size_t need_saved = tt_saved_bytes(m->nlayers, N), need = tt_scratch_bytes(N);
    if (saved_bytes < need_saved) return fail(B2H_ERR_INVALID, "saved buffer smaller than b2h_tenc_train_bytes");
    if (scratch_bytes < need)
        return fail(B2H_ERR_INVALID, "scratch smaller than b2h_tenc_train_bytes (" + std::to_string(need) + " B)");
    const int ng = 4 + 12 * m->nlayers;
    std::vector<Span> outs;
    for (int i = 0; i < ng; ++i) {
        if (!grads[i]) return fail(B2H_ERR_INVALID, "grads[" + std::to_string(i) + "] is NULL");
        if (misaligned(grads[i], 4)) return fail(B2H_ERR_INVALID, "grads must be 4-byte aligned");
        outs.push_back({grads[i], m->sizes[i + 1] * 4});
    }
    if (dx) outs.push_back({dx, (size_t)N * kInCh * 4});
    outs.push_back({scratch, need});
    if (int rc = check_overlap(outs, tt_read_only(params, m->sizes, masks, tenc_mask_bytes(m, B, T),
                                                  {{dy, (size_t)N * kOutCh * 4}, {saved, need_saved}})))
        return rc;

    hipStream_t st = (hipStream_t)stream;
    const TtLin ln{st, tenc_train_linear_mfma(m)};
    const TrainAttn attn = tenc_train_attn(m);
    const float sc = tt_scale(p);
    auto mk = [&](int i) { return masks ? masks[i] : nullptr; };
    float* S = const_cast<float*>(static_cast<const float*>(saved)); // read only
    const TtGrad G = tt_grad(static_cast<float*>(scratch), N);
    const float* X0 = S;
    const float* H0 = S + N * kInCh;
    float* Ls = S + N * kTtSavedFrame;
    // hidden2pose_projection (HandPoseModels.py:173)
    const int oh = 3 + 12 * m->nlayers;
    const float* Hlast = tt_layer(Ls, N, m->nlayers - 1).H2;
    tt_linear_dw(ln, dy, Hlast, G.slabs, N, kTtD, kOutCh, grads[oh - 1], grads[oh]);
    tt_linear_dx(ln, dy, params[oh], G.gA, N, kTtD, kOutCh, nullptr, nullptr, 1.f, nullptr);
    for (int l = m->nlayers - 1; l >= 0; --l)
        tt_enc_layer_backward(ln, attn, params + 3 + 12 * l, grads + 2 + 12 * l, tt_layer(Ls, N, l),
                              l ? tt_layer(Ls, N, l - 1).H2 : H0, G, B, (int)T, masks ? masks + 1 + 4 * l : nullptr, sc,
                              nullptr);
    // pose2hidden_projection (:171) and the positional encoding's dropout (:101-103)
    tt_linear_dw(ln, G.gA, X0, G.slabs, N, kInCh, kTtD, grads[0], grads[1]);
    if (dx) tt_linear_dx(ln, G.gA, params[1], dx, N, kInCh, kTtD, nullptr, mk(0), sc, nullptr);
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

} // extern "C"

// ---- TextPoseTransformer training (kernel_tpt_train.h) --------------------------------------------------------
// torch.nn.Transformer in .train() mode between token_embedding and the two pose projections
// (HandPoseModels.py:201-222 under autograd).  Ns = B*S token rows, Nt = B*T frame rows.
namespace {

// Saved activations (floats).  Token rows: E0 (the embeddings), every encoder layer as TransformerEnc saves it,
// MEM (encoder.norm's output) with {mean, rstd, -, -}, and [K | V] of MEM per decoder layer.  Frame rows: X0 (a
// copy of x, which the backward does not receive), XT0 (pose2hidden_projection), every decoder layer, YN
// (decoder.norm's output) with its statistics.
constexpr int64_t kTptSavedToken = 2 * kTtD + 4, kTptSavedTokenDec = 2 * kTtD;
constexpr int64_t kTptSavedFrame = 2 * kTtD + 4; // + X0: the model's ninp rounded up to a float4 (tpt_x0_ld)
constexpr int64_t kTptSavedFrameDec = 3 * kTtD + 10 * kTtD + 8; // QKV, O, R1, H1, QC, OC, R2, H2, F1, R3, H3, statistics
// Backward scratch: TtGrad over max(Ns, Nt) rows, then per token [dK | dV] and two dMEM rows (the sum over the
// decoder layers alternates between them), then the slabs.
constexpr int64_t kTptScratchToken = 2 * kTtD + 2 * kTtD;
// Beyond 128 frames (kernel_train_attn_long.h) the two attentions of every decoder layer also save their rows'
// log-sum-exp, (B, 4, T) each, behind everything else, and the backward keeps the row terms {D, sigma},
// (B, 4, T, 2), behind the slabs.  Nothing is added at T <= 128.
constexpr int64_t kTptSavedFrameLong = 2 * kTtHeads, kTptScratchFrameLong = 2 * kTtHeads;
bool tpt_long(int64_t T) { return T > kTptMaxLen; }

int64_t tpt_x0_ld(const b2h_tpt* m) { return (m->ninp + 3) / 4 * 4; } // keeps XT0 .. 16-byte aligned

struct TptDecLayer {
    float *QKV, *O, *R1, *H1, *QC, *OC, *R2, *H2, *F1, *R3, *H3, *ST12, *ST3, *KV;
};
struct TptSaved {
    float *E0, *enc, *MEM, *STm, *KV, *X0, *XT0, *dec, *YN, *STy, *LSE;
    int64_t Ns, Nt;
    TtLayer enc_layer(int l) const { return tt_layer(enc, Ns, l); }
    const float* enc_out(int n_enc) const { return enc_layer(n_enc - 1).H2; }
    TptDecLayer dec_layer(int l) const {
        float* p = dec + (int64_t)l * Nt * kTptSavedFrameDec;
        const int64_t D = Nt * kTtD;
        return TptDecLayer{p, p + 3 * D, p + 4 * D, p + 5 * D, p + 6 * D, p + 7 * D, p + 8 * D, p + 9 * D, p + 10 * D,
                           p + 11 * D, p + 12 * D, p + 13 * D, p + 13 * D + 4 * Nt, KV + (int64_t)l * Ns * kTptSavedTokenDec};
    }
};
TptSaved tpt_saved(const b2h_tpt* m, void* saved, int64_t Ns, int64_t Nt) {
    TptSaved s;
    s.Ns = Ns; s.Nt = Nt;
    s.E0 = static_cast<float*>(saved);
    s.enc = s.E0 + Ns * kTtD;
    s.MEM = s.enc + Ns * kTtSavedLayer * m->n_enc;
    s.STm = s.MEM + Ns * kTtD;
    s.KV = s.STm + Ns * 4;
    s.X0 = s.KV + Ns * kTptSavedTokenDec * m->n_dec;
    s.XT0 = s.X0 + Nt * tpt_x0_ld(m); // X0 itself is (Nt, ninp), dense
    s.dec = s.XT0 + Nt * kTtD;
    s.YN = s.dec + Nt * kTptSavedFrameDec * m->n_dec;
    s.STy = s.YN + Nt * kTtD;
    s.LSE = s.STy + Nt * 4; // long T only: per decoder layer the self-attention's rows, then the cross-attention's
    return s;
}

size_t tpt_saved_bytes(const b2h_tpt* m, int64_t Ns, int64_t Nt, bool lng) {
    return ((size_t)Ns * (kTptSavedToken + m->n_enc * kTtSavedLayer + m->n_dec * kTptSavedTokenDec) +
            (size_t)Nt * (tpt_x0_ld(m) + kTptSavedFrame + m->n_dec * (kTptSavedFrameDec + (lng ? kTptSavedFrameLong : 0)))) * 4;
}
size_t tpt_scratch_bytes(int64_t Ns, int64_t Nt, bool lng) {
    const int64_t Nmax = std::max(Ns, Nt);
    return ((size_t)Nmax * kTtScratchFrame + (size_t)Ns * kTptScratchToken + (size_t)tt_nslabs(Nmax) * kTtSlab +
            (lng ? (size_t)Nt * kTptScratchFrameLong : 0)) * 4;
}

int tpt_nparams(const b2h_tpt* m) { return 9 + 12 * m->n_enc + 18 * m->n_dec; }
int tpt_nmasks(const b2h_tpt* m) { return 4 * m->n_enc + 6 * m->n_dec; }

// Elements of every keep-mask, in the order of `masks`: per encoder layer attn, drop1, ff, drop2; per decoder layer
// self_attn, drop1, cross_attn, drop2, ff, drop3.
std::vector<size_t> tpt_mask_bytes(const b2h_tpt* m, int64_t B, int64_t S, int64_t T) {
    std::vector<size_t> n(tpt_nmasks(m), (size_t)B * T * kTtD);
    for (int i = 0; i < 4 * m->n_enc; ++i) n[i] = i % 4 == 0 ? (size_t)B * kTtHeads * S * S : (size_t)B * S * kTtD;
    for (size_t i = 4 * m->n_enc; i < n.size(); i += 6) {
        n[i] = (size_t)B * kTtHeads * T * T;
        n[i + 2] = (size_t)B * kTtHeads * T * S;
    }
    return n;
}

// Why the training calls refuse a (B, S, T) batch, or nullptr (b2h_tpt_mask_numel answers the same shapes).
const char* tptt_shape_refusal(int64_t B, int64_t S, int64_t T) {
    if (B < 0 || S < 1 || T < 1) return "expected B >= 0, S >= 1 and T >= 1";
    if (S > kTptMaxLen || T > B2H_TPT_MAX_FRAMES)
        return "TextPoseTransformer training: S is limited to 128 and T to B2H_TPT_MAX_FRAMES = 1024";
    // grid limits: attention launches B x heads workgroups, LayerNorm N / 4 (the largest row grid)
    if (B * kTtHeads > 0x7fffffff || B * std::max(S, T) / 4 >= 0x7fffffff) return "batch too large for one launch";
    return nullptr;
}

// Checks shared by b2h_tpt_train_forward_masked / b2h_tpt_backward_masked: tt_check's, then the token ids and the key
// lengths.
int tptt_check(const b2h_tpt* m, const float* const* params, const int64_t* tokens, const uint8_t* const* masks, float p,
               int64_t B, int64_t S, int64_t T, const int64_t* text_len, const int64_t* frame_len) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    if (int rc = tt_check(tptt_shape_refusal(B, S, T), params, tpt_nparams(m), masks, tpt_nmasks(m), p)) return rc;
    if (B > 0 && !tokens) return fail(B2H_ERR_INVALID, "tokens is NULL");
    if (misaligned(tokens, 8)) return fail(B2H_ERR_INVALID, "tokens must be 8-byte aligned");
    if (misaligned(text_len, 8) || misaligned(frame_len, 8))
        return fail(B2H_ERR_INVALID, "text_len and frame_len must be 8-byte aligned int64 arrays");
    return B2H_OK;
}

// The key lengths of a training call among its read-only operands (check_overlap)
void tptt_add_lengths(std::vector<Span>& ins, const int64_t* text_len, const int64_t* frame_len, int64_t B) {
    if (text_len) ins.push_back({text_len, (size_t)B * 8, "a key length array"});
    if (frame_len) ins.push_back({frame_len, (size_t)B * 8, "a key length array"});
}

void tt_layernorm(hipStream_t st, const float* X, const float* gamma, const float* beta, float* Y, float* stats, int64_t N) {
    hipLaunchKernelGGL(b2h_tt_layernorm, dim3(tt_row_blocks(N, 4)), dim3(256), 0, st, X, gamma, beta, Y, stats, 4, N);
}

// Which kernels run the decoder's two attentions in training: a whole-matrix pair up to 128 frames, as
// b2h_tpt_set_train_whole chose, beyond them the blocked ones as b2h_tpt_set_train_kernel chose.  The one place that
// decides: the dispatch and b2h_tpt_train_attn_name both ask it.
TrainAttn tpt_train_attn(const b2h_tpt* m, int64_t T) {
    if (!tpt_long(T)) return m->train_whole == B2H_TRAIN_MFMA ? TrainAttn::kWholeMfma : TrainAttn::kWhole;
    return m->train_kernel == B2H_TRAIN_MFMA ? TrainAttn::kBlockedMfma : TrainAttn::kBlockedValu;
}

// Which whole-matrix pair runs the encoder's self-attention (S <= 128 tokens at every T), as b2h_tpt_set_train_whole
// chose: the dispatch and b2h_tpt_train_enc_attn_name both ask it.
TrainAttn tpt_train_enc_attn(const b2h_tpt* m) {
    return m->train_whole == B2H_TRAIN_MFMA ? TrainAttn::kWholeMfma : TrainAttn::kWhole;
}

// Which Linear trio the training calls launch, as b2h_tpt_set_train_linear chose, at every (B, S, T): the one place
// that decides; the dispatch and b2h_tpt_train_linear_name both ask it.
enum class TrainLinear { kValu, kMfma };
TrainLinear tpt_train_linear(const b2h_tpt* m) {
    return m->train_linear == B2H_TRAIN_MFMA ? TrainLinear::kMfma : TrainLinear::kValu;
}

} // namespace

extern "C" {

const char* b2h_tpt_train_attn_name(const b2h_tpt* m, int64_t T) {
    if (!m || T < 1) return nullptr;
    switch (tpt_train_attn(m, T)) {
    case TrainAttn::kWhole: return "b2h_tt_sdpa";
    case TrainAttn::kWholeMfma: return "b2h_mw_sdpa";
    case TrainAttn::kBlockedValu: return "b2h_lt_sdpa";
    default: return "b2h_mt_sdpa";
    }
}

const char* b2h_tpt_train_enc_attn_name(const b2h_tpt* m) {
    if (!m) return nullptr;
    return tpt_train_enc_attn(m) == TrainAttn::kWholeMfma ? "b2h_mw_sdpa" : "b2h_tt_sdpa";
}

const char* b2h_tpt_train_linear_name(const b2h_tpt* m) {
    if (!m) return nullptr;
    return tpt_train_linear(m) == TrainLinear::kMfma ? "b2h_ml_linear" : "b2h_tt_linear";
}

size_t b2h_tpt_train_bytes(const b2h_tpt* m, int64_t B, int64_t S, int64_t T, int which) {
    if (!m || B < 1 || S < 1 || T < 1 || (which != 0 && which != 1)) return 0;
    return which == 0 ? tpt_saved_bytes(m, B * S, B * T, tpt_long(T)) : tpt_scratch_bytes(B * S, B * T, tpt_long(T));
}

int b2h_tpt_train_forward_masked(b2h_tpt* m, const float* const* params, const int64_t* tokens, const float* x,
                                 const uint8_t* const* masks, float p, float* y, void* saved, size_t saved_bytes, int64_t B,
                                 int64_t S, int64_t T, const int64_t* text_len, const int64_t* frame_len, void* stream) {
    if (int rc = tptt_check(m, params, tokens, masks, p, B, S, T, text_len, frame_len)) return rc;
    if (B == 0) return B2H_OK;
    if (!x || !y || !saved) return fail(B2H_ERR_INVALID, "NULL pointer");
    if (int rc = check_device(m->device)) return rc;
    if (misaligned(x, 16) || misaligned(y, 16) || misaligned(saved, 16))
        return fail(B2H_ERR_INVALID, "x, y and the saved buffer must be 16-byte aligned");
    const int64_t Ns = B * S, Nt = B * T;
    const bool lng = tpt_long(T);
    const TrainAttn route = tpt_train_attn(m, T);
    const size_t need = tpt_saved_bytes(m, Ns, Nt, lng);
    if (saved_bytes < need)
        return fail(B2H_ERR_INVALID, "saved buffer smaller than b2h_tpt_train_bytes (" + std::to_string(need) + " B)");
    std::vector<Span> ins = tt_read_only(params, tpt_param_floats(m), masks, tpt_mask_bytes(m, B, S, T),
                                         {{tokens, (size_t)Ns * 8}, {x, (size_t)Nt * m->ninp * 4}});
    tptt_add_lengths(ins, text_len, frame_len, B);
    if (int rc = check_overlap({{y, (size_t)Nt * m->nout * 4}, {saved, need}}, ins)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const TtLin ln{st, tpt_train_linear(m) == TrainLinear::kMfma};
    const float sc = tt_scale(p);
    const auto mk = [&](int i) { return masks ? masks[i] : nullptr; };
    const TptSaved sv = tpt_saved(m, saved, Ns, Nt);

    // encoder: token_embedding (:206) -> layers -> encoder.norm
    const float* const* wt = params + 4 + 12 * m->n_enc + 18 * m->n_dec; // token_embedding, hidden2pose, pose2hidden
    // the caller's table is promised 4-byte aligned only: float4 reads on the 16-byte grid, dwords off it
    hipLaunchKernelGGL(misaligned(wt[0], 16) ? b2h_embed_dwords : b2h_tpt_embed,
                       dim3((unsigned)((Ns * 32 + 255) / 256)), dim3(256), 0, st, tokens, wt[0], sv.E0, Ns, m->n_tokens);
    const float* H = sv.E0;
    for (int l = 0; l < m->n_enc; ++l) {
        const TtLayer L = sv.enc_layer(l);
        tt_enc_layer_forward(ln, tpt_train_enc_attn(m), params + 12 * l, L, H, B, (int)S, masks ? masks + 4 * l : nullptr,
                             sc, text_len);
        H = L.H2;
    }
    const float* const* wn = params + 12 * m->n_enc;
    tt_layernorm(st, H, wn[0], wn[1], sv.MEM, sv.STm, Ns);

    // decoder: pose2hidden_projection (:209) -> layers -> decoder.norm -> hidden2pose_projection (:213)
    HIP_TRY(hipMemcpyAsync(sv.X0, x, (size_t)Nt * m->ninp * 4, hipMemcpyDeviceToDevice, st));
    tt_linear(ln, sv.X0, wt[3], wt[4], sv.XT0, Nt, m->ninp, kTtD, 0, nullptr, 1.f, nullptr);
    H = sv.XT0;
    for (int l = 0; l < m->n_dec; ++l) { // torch.nn.TransformerDecoderLayer, post-norm, ReLU
        const float* const* w = params + 12 * m->n_enc + 2 + 18 * l;
        const int mi = 4 * m->n_enc + 6 * l;
        const TptDecLayer L = sv.dec_layer(l);
        tt_linear(ln, H, w[0], w[1], L.QKV, Nt, kTtD, 3 * kTtD, 0, nullptr, 1.f, nullptr);
        float* lse = sv.LSE + (int64_t)l * Nt * kTptSavedFrameLong; // long T only
        train_sdpa(st, route, self_src(L.QKV), mk(mi), sc, L.O, lse, B, (int)T, (int)T, frame_len);
        tt_linear(ln, L.O, w[2], w[3], L.R1, Nt, kTtD, kTtD, 0, mk(mi + 1), sc, H);
        tt_layernorm(st, L.R1, w[12], w[13], L.H1, L.ST12, Nt);
        // multihead_attn: the query of H1 (in_proj rows 0..127), [K | V] of the memory (rows 128..383)
        tt_linear(ln, L.H1, w[4], w[5], L.QC, Nt, kTtD, kTtD, 0, nullptr, 1.f, nullptr);
        tt_linear(ln, sv.MEM, w[4] + kDD, w[5] + kTtD, L.KV, Ns, kTtD, 2 * kTtD, 0, nullptr, 1.f, nullptr);
        train_sdpa(st, route, cross_src(L.QC, L.KV), mk(mi + 2), sc, L.OC, lse + Nt * kTtHeads, B, (int)T, (int)S, text_len);
        tt_linear(ln, L.OC, w[6], w[7], L.R2, Nt, kTtD, kTtD, 0, mk(mi + 3), sc, L.H1);
        tt_layernorm(st, L.R2, w[14], w[15], L.H2, L.ST12 + 2, Nt);
        tt_linear(ln, L.H2, w[8], w[9], L.F1, Nt, kTtD, kTtD, 1, mk(mi + 4), sc, nullptr);
        tt_linear(ln, L.F1, w[10], w[11], L.R3, Nt, kTtD, kTtD, 0, mk(mi + 5), sc, L.H2);
        tt_layernorm(st, L.R3, w[16], w[17], L.H3, L.ST3, Nt);
        H = L.H3;
    }
    const float* const* wd = params + 12 * m->n_enc + 2 + 18 * m->n_dec;
    tt_layernorm(st, H, wd[0], wd[1], sv.YN, sv.STy, Nt);
    tt_linear(ln, sv.YN, wt[1], wt[2], y, Nt, kTtD, m->nout, 0, nullptr, 1.f, nullptr);
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

int b2h_tpt_train_forward(b2h_tpt* m, const float* const* params, const int64_t* tokens, const float* x,
                          const uint8_t* const* masks, float p, float* y, void* saved, size_t saved_bytes, int64_t B,
                          int64_t S, int64_t T, void* stream) {
    return b2h_tpt_train_forward_masked(m, params, tokens, x, masks, p, y, saved, saved_bytes, B, S, T, nullptr, nullptr,
                                        stream);
}

int b2h_tpt_backward_masked(b2h_tpt* m, const float* const* params, const int64_t* tokens, const uint8_t* const* masks,
                            float p, const float* dy, const void* saved, size_t saved_bytes, float* dx, float* const* grads,
                            void* scratch, size_t scratch_bytes, int64_t B, int64_t S, int64_t T, const int64_t* text_len,
                            const int64_t* frame_len, void* stream) {
    if (int rc = tptt_check(m, params, tokens, masks, p, B, S, T, text_len, frame_len)) return rc;
    if (B == 0) return fail(B2H_ERR_SHAPE, "b2h_tpt_backward needs B >= 1 (the gradients of an empty batch are not defined here)");
    if (!dy || !saved || !scratch) return fail(B2H_ERR_INVALID, "dy / saved / scratch is NULL");
    if (!grads) return fail(B2H_ERR_INVALID, "grads is NULL");
    if (int rc = check_device(m->device)) return rc;
    if (misaligned(dy, 16) || misaligned(saved, 16) || misaligned(scratch, 16) || (dx && misaligned(dx, 16)))
        return fail(B2H_ERR_INVALID, "dy, dx, the saved buffer and the scratch must be 16-byte aligned");
    const int64_t Ns = B * S, Nt = B * T;
    const bool lng = tpt_long(T);
    const TrainAttn route = tpt_train_attn(m, T);
    const size_t need_saved = tpt_saved_bytes(m, Ns, Nt, lng), need = tpt_scratch_bytes(Ns, Nt, lng);
    if (saved_bytes < need_saved) return fail(B2H_ERR_INVALID, "saved buffer smaller than b2h_tpt_train_bytes");
    if (scratch_bytes < need)
        return fail(B2H_ERR_INVALID, "scratch smaller than b2h_tpt_train_bytes (" + std::to_string(need) + " B)");
    const std::vector<size_t> sizes = tpt_param_floats(m);
    std::vector<Span> outs;
    for (size_t i = 0; i < sizes.size(); ++i) {
        if (!grads[i]) return fail(B2H_ERR_INVALID, "grads[" + std::to_string(i) + "] is NULL");
        if (misaligned(grads[i], 4)) return fail(B2H_ERR_INVALID, "grads must be 4-byte aligned");
        outs.push_back({grads[i], sizes[i] * 4});
    }
    if (dx) outs.push_back({dx, (size_t)Nt * m->ninp * 4});
    outs.push_back({scratch, need});
    std::vector<Span> ins = tt_read_only(params, sizes, masks, tpt_mask_bytes(m, B, S, T),
                                         {{tokens, (size_t)Ns * 8}, {dy, (size_t)Nt * m->nout * 4}, {saved, need_saved}});
    tptt_add_lengths(ins, text_len, frame_len, B);
    if (int rc = check_overlap(outs, ins)) return rc;

    hipStream_t st = (hipStream_t)stream;
    const TtLin ln{st, tpt_train_linear(m) == TrainLinear::kMfma};
    const float sc = tt_scale(p);
    const auto mk = [&](int i) { return masks ? masks[i] : nullptr; };
    const TptSaved sv = tpt_saved(m, const_cast<void*>(saved), Ns, Nt); // read only
    const int64_t Nmax = std::max(Ns, Nt);
    float* scr = static_cast<float*>(scratch);
    float* dKV = scr + Nmax * kTtScratchFrame;
    float* dM[2] = {dKV + Ns * 2 * kTtD, dKV + Ns * 3 * kTtD};
    TtGrad G = tt_grad(scr, Nt); // the frame rows first; the slabs lie behind both row sets
    G.slabs = dM[1] + Ns * kTtD;
    float* Drow = G.slabs + (int64_t)tt_nslabs(Nmax) * kTtSlab; // long T only
    const int od = 12 * m->n_enc + 2, ot = od + 18 * m->n_dec + 2; // the first decoder layer; token_embedding

    // hidden2pose_projection (:213) and decoder.norm
    tt_linear_dw(ln, dy, sv.YN, G.slabs, Nt, kTtD, m->nout, grads[ot + 1], grads[ot + 2]);
    tt_linear_dx(ln, dy, params[ot + 1], G.gB, Nt, kTtD, m->nout, nullptr, nullptr, 1.f, nullptr);
    tt_layernorm_bwd(st, G.gB, sv.dec_layer(m->n_dec - 1).H3, sv.STy, params[ot - 2], G.gA, G.gBm, nullptr, 1.f, G.slabs, Nt,
                     grads[ot - 2], grads[ot - 1]);
    float* dMEM = nullptr; // the sum over the decoder layers done so far
    for (int l = m->n_dec - 1; l >= 0; --l) {
        const float* const* w = params + od + 18 * l;
        float* const* g = grads + od + 18 * l;
        const int mi = 4 * m->n_enc + 6 * l;
        const TptDecLayer L = sv.dec_layer(l);
        const float* Hin = l ? sv.dec_layer(l - 1).H3 : sv.XT0;
        // norm3: gA = dH3 -> gB = dR3 (also dH2 through the residual), gBm = dR3 through drop3
        tt_layernorm_bwd(st, G.gA, L.R3, L.ST3, w[16], G.gB, G.gBm, mk(mi + 5), sc, G.slabs, Nt, g[16], g[17]);
        const float* dF = masks ? G.gBm : G.gB;
        tt_linear_dw(ln, dF, L.F1, G.slabs, Nt, kTtD, kTtD, g[10], g[11]);
        tt_linear_dx(ln, dF, w[10], G.gC, Nt, kTtD, kTtD, L.F1, nullptr, masks ? sc : 1.f, nullptr); // through drop_ff and ReLU
        tt_linear_dw(ln, G.gC, L.H2, G.slabs, Nt, kTtD, kTtD, g[8], g[9]);
        tt_linear_dx(ln, G.gC, w[8], G.gA, Nt, kTtD, kTtD, nullptr, nullptr, 1.f, G.gB);             // gA = dH2
        // norm2: gA -> gB = dR2 (also dH1 through the residual), gBm through drop2
        tt_layernorm_bwd(st, G.gA, L.R2, L.ST12 + 2, w[14], G.gB, G.gBm, mk(mi + 3), sc, G.slabs, Nt, g[14], g[15]);
        const float* dC = masks ? G.gBm : G.gB;
        tt_linear_dw(ln, dC, L.OC, G.slabs, Nt, kTtD, kTtD, g[6], g[7]);
        tt_linear_dx(ln, dC, w[6], G.gC, Nt, kTtD, kTtD, nullptr, nullptr, 1.f, nullptr);            // gC = dOC
        const float* lse = sv.LSE + (int64_t)l * Nt * kTptSavedFrameLong; // long T only
        train_sdpa_bwd(st, route, cross_src(L.QC, L.KV), G.gC, lse + Nt * kTtHeads, Drow, mk(mi + 2), sc,
                       LtGradDst{G.gA, kTtD, 0, dKV, 2 * kTtD, 0, kTtD}, B, (int)T, (int)S, text_len); // gA = dQC, dKV
        // multihead_attn.in_proj: rows 0..127 from (dQC, H1) over the frames, rows 128..383 from ([dK | dV], MEM)
        // over the tokens, each with the slab count of its own row set
        tt_linear_dw(ln, G.gA, L.H1, G.slabs, Nt, kTtD, kTtD, g[4], g[5]);
        tt_linear_dw(ln, dKV, sv.MEM, G.slabs, Ns, kTtD, 2 * kTtD, g[4] + kDD, g[5] + kTtD);
        tt_linear_dx(ln, G.gA, w[4], G.gC, Nt, kTtD, kTtD, nullptr, nullptr, 1.f, G.gB);             // gC = dH1
        float* dMnext = dMEM == dM[0] ? dM[1] : dM[0];
        tt_linear_dx(ln, dKV, w[4] + kDD, dMnext, Ns, kTtD, 2 * kTtD, nullptr, nullptr, 1.f, dMEM);  // dMEM += [dK | dV] W_kv
        dMEM = dMnext;
        // norm1: gC -> gB = dR1 (also dH_in through the residual), gBm through drop1
        tt_layernorm_bwd(st, G.gC, L.R1, L.ST12, w[12], G.gB, G.gBm, mk(mi + 1), sc, G.slabs, Nt, g[12], g[13]);
        const float* dA = masks ? G.gBm : G.gB;
        tt_linear_dw(ln, dA, L.O, G.slabs, Nt, kTtD, kTtD, g[2], g[3]);
        tt_linear_dx(ln, dA, w[2], G.gC, Nt, kTtD, kTtD, nullptr, nullptr, 1.f, nullptr);            // gC = dO
        train_sdpa_bwd(st, route, self_src(L.QKV), G.gC, lse, Drow, mk(mi), sc, self_dst(G.gQ), B, (int)T, (int)T, frame_len);
        tt_linear_dw(ln, G.gQ, Hin, G.slabs, Nt, kTtD, 3 * kTtD, g[0], g[1]);
        tt_linear_dx(ln, G.gQ, w[0], G.gA, Nt, kTtD, 3 * kTtD, nullptr, nullptr, 1.f, G.gB);         // gA = dH_in
    }
    // pose2hidden_projection (:209)
    tt_linear_dw(ln, G.gA, sv.X0, G.slabs, Nt, m->ninp, kTtD, grads[ot + 3], grads[ot + 4]);
    if (dx) tt_linear_dx(ln, G.gA, params[ot + 3], dx, Nt, m->ninp, kTtD, nullptr, nullptr, 1.f, nullptr);

    // encoder.norm, the encoder layers, token_embedding (:206)
    float* slabs = G.slabs;
    G = tt_grad(scr, Ns);
    G.slabs = slabs;
    tt_layernorm_bwd(st, dMEM, sv.enc_out(m->n_enc), sv.STm, params[od - 2], G.gA, G.gBm, nullptr, 1.f, G.slabs, Ns,
                     grads[od - 2], grads[od - 1]);
    for (int l = m->n_enc - 1; l >= 0; --l)
        tt_enc_layer_backward(ln, tpt_train_enc_attn(m), params + 12 * l, grads + 12 * l, sv.enc_layer(l),
                              l ? sv.enc_layer(l - 1).H2 : sv.E0, G, B, (int)S, masks ? masks + 4 * l : nullptr, sc, text_len);
    hipLaunchKernelGGL(b2h_tptt_embed_bwd, dim3((unsigned)m->n_tokens), dim3(128), 0, st, tokens, G.gA, grads[ot], Ns);
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

int b2h_tpt_backward(b2h_tpt* m, const float* const* params, const int64_t* tokens, const uint8_t* const* masks, float p,
                     const float* dy, const void* saved, size_t saved_bytes, float* dx, float* const* grads, void* scratch,
                     size_t scratch_bytes, int64_t B, int64_t S, int64_t T, void* stream) {
    return b2h_tpt_backward_masked(m, params, tokens, masks, p, dy, saved, saved_bytes, dx, grads, scratch, scratch_bytes, B, S,
                                   T, nullptr, nullptr, stream);
}

} // extern "C"

// ---- dropout keep-masks (kernel_dropout_masks.h) ------------------------------------------------------------
extern "C" {

int b2h_dropout_masks(uint8_t* const* masks, const int64_t* numel, int n_masks, int first_index, float p, uint64_t seed,
                      uint64_t step, const uint64_t* step_dev, void* stream) {
    if (n_masks < 0) return fail(B2H_ERR_INVALID, "n_masks must be >= 0");
    if (first_index < 0) return fail(B2H_ERR_INVALID, "first_index must be >= 0");
    if (!(p >= 0.f && p <= 1.f)) return fail(B2H_ERR_INVALID, "dropout p must be in [0, 1]");
    if (n_masks > 0 && (!masks || !numel)) return fail(B2H_ERR_INVALID, "masks / numel is NULL");
    for (int i = 0; i < n_masks; ++i) {
        if (numel[i] < 0) return fail(B2H_ERR_INVALID, "numel[" + std::to_string(i) + "] is negative");
        if (!masks[i]) return fail(B2H_ERR_INVALID, "masks[" + std::to_string(i) + "] is NULL");
        if (misaligned(masks[i], 16)) return fail(B2H_ERR_INVALID, "masks[" + std::to_string(i) + "] must be 16-byte aligned");
    }
    DmArgs a;
    a.key0 = (uint32_t)seed;
    a.key1 = (uint32_t)(seed >> 32);
    a.thr = (uint64_t)std::ceil((double)p * 4294967296.0);
    a.step = step;
    a.step_dev = step_dev;
    for (int base = 0; base < n_masks; base += kDmMaxMasks) { // at most kDmMaxMasks masks per launch
        a.n = std::min(n_masks - base, kDmMaxMasks);
        a.number0 = (uint32_t)first_index + (uint32_t)base;
        a.first[0] = 0;
        for (int i = 0; i < kDmMaxMasks; ++i) {
            a.ptr[i] = i < a.n ? masks[base + i] : nullptr;
            a.numel[i] = i < a.n ? numel[base + i] : 0;
            a.first[i + 1] = a.first[i] + (a.numel[i] + 15) / 16;
        }
        const int64_t chunks = a.first[a.n];
        if (chunks == 0) continue;
        const unsigned blocks = (unsigned)std::min<int64_t>((chunks + kDmThreads - 1) / kDmThreads, kDmMaxBlocks);
        hipLaunchKernelGGL(b2h_dropout_masks_k, dim3(blocks), dim3(kDmThreads), 0, (hipStream_t)stream, a);
        HIP_TRY(hipGetLastError());
    }
    return B2H_OK;
}

int64_t b2h_tenc_mask_numel(const b2h_tenc* m, int64_t B, int64_t T, int64_t* numel, int capacity) {
    if (!m || tt_shape_refusal(m, B, T)) return 0;
    const std::vector<size_t> n = tenc_mask_bytes(m, B, T);
    for (int i = 0; numel && i < std::min((int)n.size(), capacity); ++i) numel[i] = (int64_t)n[i];
    return (int64_t)n.size();
}

int64_t b2h_tpt_mask_numel(const b2h_tpt* m, int64_t B, int64_t S, int64_t T, int64_t* numel, int capacity) {
    if (!m || tptt_shape_refusal(B, S, T)) return 0;
    const std::vector<size_t> n = tpt_mask_bytes(m, B, S, T);
    for (int i = 0; numel && i < std::min((int)n.size(), capacity); ++i) numel[i] = (int64_t)n[i];
    return (int64_t)n.size();
}

} // extern "C"

// ---- optimizer.step() (kernel_adam.h) ------------------------------------------------------------------------
namespace {
// The double a float hyper-parameter stands for: the shortest decimal that rounds to it, as a Python caller wrote it
// (0.999f means 0.999, not 0.99900001287).  1 - beta2 needs this: taken from the float's exact value it would be off
// by 1.3e-5 of itself, and exp_avg_sq with it.
double shortest_decimal(float x) {
    char buf[32];
    for (int digits = 1; digits <= 9; ++digits) {
        std::snprintf(buf, sizeof buf, "%.*g", digits, (double)x);
        if (std::strtof(buf, nullptr) == x) break;
    }
    return std::strtod(buf, nullptr);
}

// b2h_adam_step (guard == nullptr: b2h_adam_step_k) and b2h_adam_step_guarded (b2h_adam_guarded_k behind the two words
// of *guard): one list of refusals, one packing of the kernel arguments.
int adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
              const int64_t* numel, int n_tensors, float lr, const float* lr_dev, float beta1, float beta2, float eps,
              float weight_decay, int64_t step, const int64_t* step_dev, const AdGuard* guard, void* stream) {
    if (n_tensors < 0) return fail(B2H_ERR_INVALID, "n_tensors must be >= 0");
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return fail(B2H_ERR_INVALID, "betas must be in [0, 1)");
    if (!(eps >= 0.f)) return fail(B2H_ERR_INVALID, "eps must be >= 0");
    if (!(weight_decay >= 0.f)) return fail(B2H_ERR_INVALID, "weight_decay must be >= 0");
    if (!lr_dev && !(lr >= 0.f)) return fail(B2H_ERR_INVALID, "lr must be >= 0");
    if (step_dev ? step < 0 : step < 1)
        return fail(B2H_ERR_INVALID, "step counts from 1 (from 0 with step_dev: step + *step_dev must be >= 1)");
    if (misaligned(lr_dev, 4) || misaligned(step_dev, 8)) return fail(B2H_ERR_INVALID, "lr_dev / step_dev is misaligned");
    if (guard && (misaligned(guard->grad_scale_dev, 4) || misaligned(guard->apply_dev, 8)))
        return fail(B2H_ERR_INVALID, "grad_scale_dev / apply_dev is misaligned");
    if (n_tensors > 0 && (!params || !grads || !exp_avg || !exp_avg_sq || !numel))
        return fail(B2H_ERR_INVALID, "params / grads / exp_avg / exp_avg_sq / numel is NULL");
    for (int i = 0; i < n_tensors; ++i) {
        const std::string at = "[" + std::to_string(i) + "]";
        if (numel[i] < 0) return fail(B2H_ERR_INVALID, "numel" + at + " is negative");
        if (numel[i] == 0) continue; // the pointers of an empty tensor are never looked at
        if (numel[i] > (int64_t)1 << 40) return fail(B2H_ERR_INVALID, "numel" + at + " is too large");
        const void* ptr[4] = {params[i], grads[i], exp_avg[i], exp_avg_sq[i]};
        for (const void* q : ptr) {
            if (!q) return fail(B2H_ERR_INVALID, "a pointer of tensor " + at + " is NULL");
            if (misaligned(q, 4)) return fail(B2H_ERR_INVALID, "the pointers of tensor " + at + " must be 4-byte aligned");
        }
        const size_t bytes = (size_t)numel[i] * 4;
        for (int x = 0; x < 4; ++x)
            for (int y = x + 1; y < 4; ++y)
                if (overlaps(ptr[x], bytes, ptr[y], bytes))
                    return fail(B2H_ERR_INVALID, "params, grads, exp_avg and exp_avg_sq of tensor " + at + " overlap");
        if (guard)
            for (int x : {0, 2, 3}) // the tensors the kernel writes, against the words it reads
                if ((guard->grad_scale_dev && overlaps(ptr[x], bytes, guard->grad_scale_dev, 4)) ||
                    (guard->apply_dev && overlaps(ptr[x], bytes, guard->apply_dev, 8)))
                    return fail(B2H_ERR_INVALID, "grad_scale_dev / apply_dev lies inside an updated array of tensor " + at);
    }
    AdArgs a;
    a.b1 = shortest_decimal(beta1);
    a.b2 = shortest_decimal(beta2);
    a.w1 = (float)(1.0 - a.b1);
    a.b2f = beta2;
    a.w2 = (float)(1.0 - a.b2);
    a.eps = eps;
    a.wd = weight_decay;
    a.lr = lr;
    a.step = step;
    a.step_dev = step_dev;
    a.lr_dev = lr_dev;
    a.bc2s = a.step_size = 0.f;
    if (!step_dev && !lr_dev) ad_bias(a.b1, a.b2, (double)lr, step, &a.bc2s, &a.step_size);
    for (int base = 0; base < n_tensors; base += kAdMaxTensors) { // at most kAdMaxTensors tensors per launch
        a.n = std::min(n_tensors - base, kAdMaxTensors);
        a.first[0] = 0;
        for (int i = 0; i < kAdMaxTensors; ++i) {
            const bool used = i < a.n && numel[base + i] > 0;
            a.p[i] = used ? params[base + i] : nullptr;
            a.g[i] = used ? grads[base + i] : nullptr;
            a.m[i] = used ? exp_avg[base + i] : nullptr;
            a.v[i] = used ? exp_avg_sq[base + i] : nullptr;
            a.numel[i] = used ? numel[base + i] : 0;
            a.first[i + 1] = a.first[i] + (a.numel[i] + 3) / 4;
        }
        const int64_t chunks = a.first[a.n];
        if (chunks == 0) continue;
        const unsigned blocks = (unsigned)std::min<int64_t>((chunks + kAdThreads - 1) / kAdThreads, kAdMaxBlocks);
        if (guard)
            hipLaunchKernelGGL(b2h_adam_guarded_k, dim3(blocks), dim3(kAdThreads), 0, (hipStream_t)stream, a, *guard);
        else
            hipLaunchKernelGGL(b2h_adam_step_k, dim3(blocks), dim3(kAdThreads), 0, (hipStream_t)stream, a);
        HIP_TRY(hipGetLastError());
    }
    return B2H_OK;
}
} // namespace

extern "C" {

int b2h_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                  const int64_t* numel, int n_tensors, float lr, const float* lr_dev, float beta1, float beta2, float eps,
                  float weight_decay, int64_t step, const int64_t* step_dev, void* stream) {
    return adam_step(params, grads, exp_avg, exp_avg_sq, numel, n_tensors, lr, lr_dev, beta1, beta2, eps, weight_decay, step,
                     step_dev, nullptr, stream);
}

int b2h_adam_step_guarded(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                          const int64_t* numel, int n_tensors, float lr, const float* lr_dev, float beta1, float beta2,
                          float eps, float weight_decay, int64_t step, const int64_t* step_dev, const float* grad_scale_dev,
                          const int64_t* apply_dev, void* stream) {
    const AdGuard guard{grad_scale_dev, apply_dev};
    return adam_step(params, grads, exp_avg, exp_avg_sq, numel, n_tensors, lr, lr_dev, beta1, beta2, eps, weight_decay, step,
                     step_dev, &guard, stream);
}

// ---- between backward and the update: norm, clip, guard, warmup (kernel_step_control.h) ----------------------------
static_assert(kSchedNone == B2H_SCHED_NONE && kSchedLinear == B2H_SCHED_LINEAR && kSchedInvSqrt == B2H_SCHED_INV_SQRT,
              "kernel_step_control.h and b2h.h name the same schedules");
size_t b2h_step_prepare_bytes(const int64_t* numel, int n_tensors) {
    if (n_tensors <= 0 || !numel) return 0;
    int64_t chunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (numel[i] < 0 || numel[i] > (int64_t)1 << 40) return 0;
        chunks += (numel[i] + 3) / 4;
    }
    return (size_t)((chunks + kScBlockChunks - 1) / kScBlockChunks) * sizeof(double);
}

int b2h_step_prepare(const float* const* grads, const int64_t* numel, int n_tensors, float max_norm, int guard, float base_lr,
                     const float* base_lr_dev, int schedule, int64_t warmup_steps, int64_t step, const int64_t* step_dev,
                     float* norm_out, float* scale_out, int64_t* apply_out, int64_t* skipped, float* lr_out, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (n_tensors < 0) return fail(B2H_ERR_INVALID, "n_tensors must be >= 0");
    if (max_norm != max_norm) return fail(B2H_ERR_INVALID, "max_norm is NaN (<= 0 switches clipping off)");
    if (schedule != kSchedNone && schedule != kSchedLinear && schedule != kSchedInvSqrt)
        return fail(B2H_ERR_INVALID, "schedule must be a B2H_SCHED_* value");
    if (schedule != kSchedNone && warmup_steps < 1) return fail(B2H_ERR_INVALID, "warmup_steps must be >= 1 with a schedule");
    if (schedule != kSchedNone && (step_dev ? step < 0 : step < 1))
        return fail(B2H_ERR_INVALID, "step counts from 1 (from 0 with step_dev: step + *step_dev must be >= 1)");
    if (!base_lr_dev && !(base_lr >= 0.f)) return fail(B2H_ERR_INVALID, "base_lr must be >= 0");
    if (misaligned(base_lr_dev, 4) || misaligned(step_dev, 8)) return fail(B2H_ERR_INVALID, "base_lr_dev / step_dev is misaligned");
    if (misaligned(norm_out, 4) || misaligned(scale_out, 4) || misaligned(lr_out, 4))
        return fail(B2H_ERR_INVALID, "norm_out / scale_out / lr_out must be 4-byte aligned");
    if (misaligned(apply_out, 8) || misaligned(skipped, 8)) return fail(B2H_ERR_INVALID, "apply_out / skipped must be 8-byte aligned");
    const bool stage1 = max_norm > 0.f || guard;
    size_t need = 0;
    if (stage1 && n_tensors > 0) {
        if (!grads || !numel) return fail(B2H_ERR_INVALID, "grads / numel is NULL");
        for (int i = 0; i < n_tensors; ++i) {
            const std::string at = "[" + std::to_string(i) + "]";
            if (numel[i] < 0) return fail(B2H_ERR_INVALID, "numel" + at + " is negative");
            if (numel[i] == 0) continue; // the pointer of an empty tensor is never looked at
            if (numel[i] > (int64_t)1 << 40) return fail(B2H_ERR_INVALID, "numel" + at + " is too large");
            if (!grads[i]) return fail(B2H_ERR_INVALID, "grads" + at + " is NULL");
            if (misaligned(grads[i], 4)) return fail(B2H_ERR_INVALID, "grads" + at + " must be 4-byte aligned");
        }
        need = b2h_step_prepare_bytes(numel, n_tensors);
    }
    if (need) {
        if (!workspace) return fail(B2H_ERR_INVALID, "workspace is NULL");
        if (misaligned(workspace, 16)) return fail(B2H_ERR_INVALID, "workspace must be 16-byte aligned");
        if (workspace_bytes < need)
            return fail(B2H_ERR_INVALID, "workspace too small: " + std::to_string(workspace_bytes) + " < " + std::to_string(need) +
                                             " bytes (b2h_step_prepare_bytes)");
    }
    const Span out[6] = {{norm_out, 4, "norm_out"},  {scale_out, 4, "scale_out"}, {apply_out, 8, "apply_out"},
                         {skipped, 8, "skipped"},    {lr_out, 4, "lr_out"},       {need ? workspace : nullptr, need, "workspace"}};
    for (int x = 0; x < 6; ++x) {
        if (!out[x].p) continue;
        const std::string name = out[x].what;
        for (int y = x + 1; y < 6; ++y)
            if (out[y].p && overlaps(out[x].p, out[x].n, out[y].p, out[y].n))
                return fail(B2H_ERR_INVALID, name + " overlaps " + out[y].what);
        if ((base_lr_dev && overlaps(out[x].p, out[x].n, base_lr_dev, 4)) || (step_dev && overlaps(out[x].p, out[x].n, step_dev, 8)))
            return fail(B2H_ERR_INVALID, name + " overlaps base_lr_dev / step_dev");
        for (int i = 0; need && i < n_tensors; ++i)
            if (numel[i] > 0 && overlaps(out[x].p, out[x].n, grads[i], (size_t)numel[i] * 4))
                return fail(B2H_ERR_INVALID, name + " overlaps grads[" + std::to_string(i) + "]");
    }
    int64_t base = 0; // chunks of the call's tensors before this launch
    for (int at = 0; need && at < n_tensors; at += kScMaxTensors) { // at most kScMaxTensors tensors per launch
        SsArgs a;
        a.partial = (double*)workspace;
        a.n = std::min(n_tensors - at, kScMaxTensors);
        a.first[0] = base;
        for (int i = 0; i < kScMaxTensors; ++i) {
            const bool used = i < a.n && numel[at + i] > 0;
            a.g[i] = used ? grads[at + i] : nullptr;
            a.numel[i] = used ? numel[at + i] : 0;
            a.first[i + 1] = a.first[i] + (a.numel[i] + 3) / 4;
        }
        const int64_t end = a.first[a.n];
        if (end == base) continue;
        const int64_t blocks = (end - 1) / kScBlockChunks - base / kScBlockChunks + 1;
        hipLaunchKernelGGL(b2h_grad_sumsq_k, dim3((unsigned)std::min<int64_t>(blocks, kScMaxBlocks)), dim3(kScThreads), 0,
                           (hipStream_t)stream, a);
        HIP_TRY(hipGetLastError());
        base = end;
    }
    ScArgs c;
    c.partial = (const double*)workspace;
    c.n_partial = (int64_t)(need / sizeof(double));
    c.max_norm = (double)max_norm;
    c.base_lr = (double)base_lr;
    c.base_lr_dev = base_lr_dev;
    c.warmup = warmup_steps;
    c.step = step;
    c.step_dev = step_dev;
    c.norm_out = norm_out;
    c.scale_out = scale_out;
    c.apply_out = apply_out;
    c.skipped = skipped;
    c.lr_out = lr_out;
    c.guard = guard ? 1 : 0;
    c.schedule = schedule;
    if (!norm_out && !scale_out && !apply_out && !skipped && !lr_out) return B2H_OK; // nothing to store
    hipLaunchKernelGGL(b2h_step_control_k, dim3(1), dim3(kScThreads), 0, (hipStream_t)stream, c);
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

} // extern "C"

// ---- the training set on the device (kernel_build_batch.h) -----------------------------------------------------
namespace {

// The store and batch description b2h_build_batch and b2h_scatter_rows share: the first refusals of both, in this order.
int batch_description_refusal(int64_t n_rows, int64_t n_utt, int n_body, int64_t n_plan, int64_t B, int64_t T, int predict,
                              int flags, float factor) {
    if (B < 0 || T < 0 || n_utt < 0 || n_rows < 0 || n_plan < 0) return fail(B2H_ERR_SHAPE, "negative shape");
    if (n_body != 8 && n_body != 12) return fail(B2H_ERR_INVALID, "n_body must be 8 or 12");
    if (predict != B2H_PREDICT_RIGHT_HAND && predict != B2H_PREDICT_RIGHT_INDEX && predict != B2H_PREDICT_RIGHT_3FINGERS)
        return fail(B2H_ERR_INVALID, "predict must be a b2h_predict value");
    if (predict != B2H_PREDICT_RIGHT_HAND && n_body != 12)
        return fail(B2H_ERR_INVALID, "right_index and right_3fingers items need n_body = 12 (no model takes 25 or 17 joints)");
    if (flags & ~(kBbDif | kBbNorm | kBbPadFrame0)) return fail(B2H_ERR_INVALID, "unknown flag bits (only B2H_BATCH_* apply)");
    if ((flags & kBbNorm) && !(factor > 0.f)) return fail(B2H_ERR_INVALID, "factor must be > 0");
    return B2H_OK;
}

// What b2h_build_batch_aug adds to a build: NULL for the two plain entry points.
struct BatchAugment {
    const b2h_augment* aug;
    const uint64_t* key;
    int64_t entry0;
};

// b2h_build_batch (step NULL: utt and start hold B entries) and b2h_build_batch_planned (utt and start hold the n_plan
// entries of an epoch's plan, *step selects B of them): the same checks in the same order, the same launch.
// b2h_build_batch_aug (`with` set) is either of them with its own kernel, and its own refusals among theirs.
int build_batch(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body, const int64_t* tokens,
                int64_t S, const int64_t* utt, const int64_t* start, int64_t n_plan, const int64_t* step, bool planned,
                int64_t B, int64_t T, int predict, int flags, float factor, float* input_kp, float* target_kp,
                float* target_conf, int64_t* text_tokens, int64_t* n_frames, void* stream, const BatchAugment* with = nullptr) {
    if (int rc = batch_description_refusal(n_rows, n_utt, n_body, n_plan, B, T, predict, flags, factor)) return rc;
    if (!tokens != !text_tokens) return fail(B2H_ERR_INVALID, "tokens and text_tokens go together: both or neither");
    if (tokens && (S < 1 || S > 128)) return fail(B2H_ERR_INVALID, "1 <= S <= 128");
    if (with) {
        if (!with->aug) return fail(B2H_ERR_INVALID, "aug is NULL");
        const b2h_augment& g = *with->aug;   // each range written so that a NaN fails it
        if (!(g.scale >= 0.f && g.scale < 1.f)) return fail(B2H_ERR_INVALID, "aug.scale must be in [0, 1)");
        if (!(g.rotate_tan >= 0.f && g.rotate_tan <= 1.f)) return fail(B2H_ERR_INVALID, "aug.rotate_tan must be in [0, 1]");
        if (!(g.mirror_p >= 0.f && g.mirror_p <= 1.f)) return fail(B2H_ERR_INVALID, "aug.mirror_p must be in [0, 1]");
        if (!(g.jitter >= 0.f && std::isfinite(g.jitter))) return fail(B2H_ERR_INVALID, "aug.jitter must be finite and >= 0");
    }
    if (B * T == 0) return B2H_OK;
    if (B > 0x7fffffff || T > (1 << 24)) return fail(B2H_ERR_SHAPE, "shape too large");
    if (n_rows > ((int64_t)1 << 40) || n_utt > ((int64_t)1 << 40) || n_plan > ((int64_t)1 << 40))
        return fail(B2H_ERR_SHAPE, "store too large");
    if (with && n_plan > ((int64_t)1 << 32)) return fail(B2H_ERR_SHAPE, "plan too large (a draw index has 32 bits: n_plan <= 2^32)");
    if (with && (with->entry0 < 0 || with->entry0 > ((int64_t)1 << 32) - B))
        return fail(B2H_ERR_SHAPE, "entry0 out of range (a draw index has 32 bits: 0 <= entry0, entry0 + B <= 2^32)");
    if (!tokens) S = 0;
    const size_t entries = planned ? (size_t)n_plan : (size_t)B;
    const int J = n_body + 42;
    const int ni = predict == B2H_PREDICT_RIGHT_HAND ? n_body : predict == B2H_PREDICT_RIGHT_INDEX ? 29 : 21;
    const int nt = predict == B2H_PREDICT_RIGHT_HAND ? 21 : predict == B2H_PREDICT_RIGHT_INDEX ? 4 : 12;
    const size_t frames = (size_t)B * T;
    const Op ops[] = {{"rows", rows, (size_t)n_rows * 3 * J * 4, 8, n_rows == 0, false},
                      {"offsets", offsets, (size_t)(n_utt + 1) * 8, 8, false, false},
                      {"tokens", tokens, (size_t)n_utt * S * 8, 8, true, false},
                      {planned ? "utt_plan" : "utt", utt, entries * 8, 8, planned && n_plan == 0, false},
                      {planned ? "start_plan" : "start", start, entries * 8, 8, true, false},
                      {"step", step, 8, 8, !planned, false},
                      {"key", with ? with->key : nullptr, 16, 8, !with, false},
                      {"input_kp", input_kp, frames * ni * 8, 8, false, true},
                      {"target_kp", target_kp, frames * nt * 8, 8, false, true},
                      {"target_conf", target_conf, frames * nt * 4, 8, true, true},
                      {"text_tokens", text_tokens, (size_t)B * S * 8, 8, true, true},
                      {"n_frames", n_frames, (size_t)B * 8, 8, false, true}};
    if (int rc = check_ops(ops, true)) return rc;
    BbArgs a;
    a.rows = rows; a.offsets = offsets; a.tokens = tokens; a.utt = utt; a.start = start;
    a.input_kp = input_kp; a.target_kp = target_kp; a.target_conf = target_conf; a.text_tokens = text_tokens;
    a.n_frames = n_frames;
    a.n_rows = n_rows; a.n_utt = n_utt; a.B = B; a.T = T; a.S = S;
    a.n_body = n_body; a.predict = predict; a.flags = flags; a.ni = ni; a.nt = nt; a.factor = factor;
    a.step = planned ? step : nullptr; a.n_plan = n_plan; a.n_steps = planned ? (n_plan + B - 1) / B : 0;
    const int64_t lanes[5] = {(int64_t)frames * ni, (int64_t)frames * nt, target_conf ? (int64_t)frames * nt : 0, B * S, B};
    a.first[0] = 0;
    for (int s = 0; s < 5; ++s) a.first[s + 1] = a.first[s] + (lanes[s] + kBbThreads - 1) / kBbThreads;
    if (a.first[5] > 0x7fffffff) return fail(B2H_ERR_SHAPE, "shape too large");
    if (with) {
        BaArgs g;
        g.b = a;
        g.key = with->key; g.entry0 = with->entry0;
        g.scale = with->aug->scale; g.rotate_tan = with->aug->rotate_tan; g.jitter = with->aug->jitter;
        g.mirror_thr = (uint64_t)std::ceil((double)with->aug->mirror_p * 4294967296.0);   // exact: 24 bits times 2^32
        g.spin = g.scale != 0.f || g.rotate_tan != 0.f;
        hipLaunchKernelGGL(b2h_build_batch_aug_k, dim3((unsigned)a.first[5]), dim3(kBbThreads), 0, (hipStream_t)stream, g);
    } else {
        hipLaunchKernelGGL(b2h_build_batch_k, dim3((unsigned)a.first[5]), dim3(kBbThreads), 0, (hipStream_t)stream, a);
    }
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

// What b2h_scatter_rows_blend adds to a write-back: NULL for b2h_scatter_rows.
struct RowsBlend {
    int64_t n_plan, entry0;
    const float* pred_before;
    int blend;
};

// b2h_scatter_rows (utt, start and skip hold B entries) and b2h_scatter_rows_blend (`with` set: they hold the n_plan
// entries of a plan, of which the batch is entry0 .. entry0 + B - 1): the same checks in the same order, and the
// second's own among them.
int scatter_rows(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body, const int64_t* utt,
                 const int64_t* start, const int64_t* skip, int64_t B, int64_t T, int predict, int flags, float factor,
                 const float* pred, float conf, float* rows_out, void* stream, const RowsBlend* with = nullptr) {
    if (int rc = batch_description_refusal(n_rows, n_utt, n_body, with ? with->n_plan : 0, B, T, predict, flags, factor)) return rc;
    if (!std::isfinite(conf)) return fail(B2H_ERR_INVALID, "conf must be finite");
    if (with) {
        if (with->blend != B2H_BLEND_LINEAR && with->blend != B2H_BLEND_CENTRE)
            return fail(B2H_ERR_INVALID, "blend must be a b2h_blend value");
        if (with->entry0 < 0 || with->entry0 > with->n_plan - B)
            return fail(B2H_ERR_INVALID, "entry0 out of range (0 <= entry0, entry0 + B <= n_plan): entry0 " +
                                             std::to_string(with->entry0) + ", B " + std::to_string(B) + ", n_plan " +
                                             std::to_string(with->n_plan));
    }
    if (B * T == 0) return B2H_OK;
    if (B > 0x7fffffff || T > (1 << 24)) return fail(B2H_ERR_SHAPE, "shape too large");
    if (n_rows > ((int64_t)1 << 40) || n_utt > ((int64_t)1 << 40)) return fail(B2H_ERR_SHAPE, "store too large");
    if (with && with->n_plan > ((int64_t)1 << 40)) return fail(B2H_ERR_SHAPE, "plan too large");
    const int J = n_body + 42;
    const int nt = predict == B2H_PREDICT_RIGHT_HAND ? 21 : predict == B2H_PREDICT_RIGHT_INDEX ? 4 : 12;
    const size_t store = (size_t)n_rows * 3 * J * 4, entries = (size_t)(with ? with->n_plan : B) * 8;
    const Op ops[] = {{"rows", rows, store, 8, n_rows == 0, false},
                      {"offsets", offsets, (size_t)(n_utt + 1) * 8, 8, false, false},
                      {with ? "utt_plan" : "utt", utt, entries, 8, false, false},
                      {with ? "start_plan" : "start", start, entries, 8, !with, false},
                      {with ? "skip_plan" : "skip", skip, entries, 8, !with, false},
                      {"pred", pred, (size_t)B * T * nt * 8, 8, false, false},
                      {"pred_before", with ? with->pred_before : nullptr, (size_t)T * nt * 8, 8, true, false},
                      {"rows_out", rows_out, store, 8, n_rows == 0, true}};
    if (int rc = check_ops(ops, true)) return rc;
    SbArgs g = {};
    SrArgs& a = g.s;
    a.w.rows = rows; a.w.offsets = offsets; a.w.utt = utt; a.w.start = start;
    a.w.n_rows = n_rows; a.w.n_utt = n_utt; a.w.B = B; a.w.T = T;
    a.w.n_body = n_body; a.w.predict = predict; a.w.flags = flags; a.w.nt = nt; a.w.factor = factor;
    a.skip = skip; a.pred = pred; a.rows_out = rows_out; a.conf = conf;
    const int64_t blocks = (B * T * nt + kBbThreads - 1) / kBbThreads;
    if (blocks > 0x7fffffff) return fail(B2H_ERR_SHAPE, "shape too large");
    if (with) {
        g.before = with->pred_before; g.entry0 = with->entry0; g.n_plan = with->n_plan; g.blend = with->blend;
        hipLaunchKernelGGL(b2h_scatter_rows_blend_k, dim3((unsigned)blocks), dim3(kBbThreads), 0, (hipStream_t)stream, g);
    } else {
        hipLaunchKernelGGL(b2h_scatter_rows_k, dim3((unsigned)blocks), dim3(kBbThreads), 0, (hipStream_t)stream, a);
    }
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

// b2h_window_plan (overlap 0) and b2h_window_plan_overlap: windows at stride T - overlap, the last a full window that
// ends with the utterance.  With overlap 0 that is ceil(L / T) windows at i T and (L - T, k T - L).
int64_t window_plan(const int64_t* offsets, int64_t n_utt, int64_t T, int coverage, int64_t overlap, int64_t* utt_plan,
                    int64_t* start_plan, int64_t* skip_plan, int64_t capacity) {
    const auto refuse = [](const std::string& why) {
        (void)fail(B2H_ERR_INVALID, why);
        return (int64_t)-1;
    };
    if (T < 1) return refuse("T must be >= 1");
    if (n_utt < 0 || capacity < 0) return refuse("negative shape");
    if (coverage != B2H_COVER_ALL && coverage != B2H_COVER_FIRST) return refuse("coverage must be a b2h_coverage value");
    if (!offsets && n_utt > 0) return refuse("offsets is NULL");
    if (n_utt > 0 && offsets[0] < 0) return refuse("offsets must ascend from offsets[0] >= 0");
    for (int64_t u = 0; u < n_utt; ++u)
        if (offsets[u + 1] < offsets[u]) return refuse("offsets must ascend from offsets[0] >= 0");
    if (overlap < 0 || overlap > T / 2)
        return refuse("overlap must be in 0 .. T / 2 (a frame is predicted by at most two windows): overlap " +
                      std::to_string(overlap) + ", T " + std::to_string(T));
    const int64_t stride = T - overlap;               // >= 1
    int64_t count = 0;
    for (int64_t u = 0; u < n_utt; ++u) {
        const int64_t L = offsets[u + 1] - offsets[u];
        if (L == 0) continue;
        const int64_t k = (coverage == B2H_COVER_FIRST || L <= T) ? 1 : (L - T + stride - 1) / stride + 1;
        for (int64_t i = 0; i < k; ++i, ++count) {
            if (count >= capacity) continue;
            if (!utt_plan || !start_plan || !skip_plan) return refuse("utt_plan, start_plan or skip_plan is NULL");
            const bool last = k > 1 && i == k - 1;    // a full window that ends with the utterance
            utt_plan[count] = u;
            start_plan[count] = last ? L - T : i * stride;
            skip_plan[count] = last ? i * stride - (L - T) : 0;
        }
    }
    return count;
}

} // namespace

extern "C" {

int b2h_build_batch(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body,
                    const int64_t* tokens, int64_t S, const int64_t* utt, const int64_t* start, int64_t B, int64_t T,
                    int predict, int flags, float factor, float* input_kp, float* target_kp, float* target_conf,
                    int64_t* text_tokens, int64_t* n_frames, void* stream) {
    return build_batch(rows, n_rows, offsets, n_utt, n_body, tokens, S, utt, start, 0, nullptr, false, B, T, predict, flags,
                       factor, input_kp, target_kp, target_conf, text_tokens, n_frames, stream);
}

int b2h_build_batch_planned(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body,
                            const int64_t* tokens, int64_t S, const int64_t* utt_plan, const int64_t* start_plan,
                            int64_t n_plan, const int64_t* step, int64_t B, int64_t T, int predict, int flags, float factor,
                            float* input_kp, float* target_kp, float* target_conf, int64_t* text_tokens, int64_t* n_frames,
                            void* stream) {
    return build_batch(rows, n_rows, offsets, n_utt, n_body, tokens, S, utt_plan, start_plan, n_plan, step, true, B, T,
                       predict, flags, factor, input_kp, target_kp, target_conf, text_tokens, n_frames, stream);
}

int b2h_build_batch_aug(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body,
                        const int64_t* tokens, int64_t S, const int64_t* utt, const int64_t* start, int64_t n_plan,
                        const int64_t* step, int64_t entry0, const b2h_augment* aug, const uint64_t* key, int64_t B, int64_t T,
                        int predict, int flags, float factor, float* input_kp, float* target_kp, float* target_conf,
                        int64_t* text_tokens, int64_t* n_frames, void* stream) {
    const BatchAugment with = {aug, key, entry0};
    const bool planned = step != nullptr;   // without a step word utt and start hold B entries and n_plan is not looked at
    return build_batch(rows, n_rows, offsets, n_utt, n_body, tokens, S, utt, start, planned ? n_plan : 0, step, planned, B, T,
                       predict, flags, factor, input_kp, target_kp, target_conf, text_tokens, n_frames, stream, &with);
}

// ---- an epoch's plan and its step word (kernel_epoch_plan.h) ---------------------------------------------------
int b2h_epoch_plan(const int64_t* offsets, int64_t n_utt, int64_t T, int shuffle, int random_crop, uint64_t seed,
                   uint64_t epoch, int64_t* utt_plan, int64_t* start_plan, void* stream) {
    if (n_utt < 0 || T < 0) return fail(B2H_ERR_SHAPE, "negative shape");
    if (n_utt > ((int64_t)1 << 30)) return fail(B2H_ERR_SHAPE, "store too large (a plan holds at most 2^30 utterances)");
    if ((shuffle != 0 && shuffle != 1) || (random_crop != 0 && random_crop != 1))
        return fail(B2H_ERR_INVALID, "shuffle and random_crop must be 0 or 1");
    if (random_crop && !start_plan) return fail(B2H_ERR_INVALID, "start_plan is NULL (it may be only without random_crop)");
    if (!utt_plan && n_utt > 0) return fail(B2H_ERR_INVALID, "utt_plan is NULL");
    if (random_crop && !offsets && n_utt > 0) return fail(B2H_ERR_INVALID, "offsets is NULL");
    if (!random_crop) offsets = nullptr;   // not read
    const size_t plan = (size_t)n_utt * 8;
    // every operand optional: what may be NULL was settled above, with messages of this entry point's own
    const Op ops[] = {{"offsets", offsets, (size_t)(n_utt + 1) * 8, 8, true, false},
                      {"utt_plan", utt_plan, plan, 8, true, true},
                      {"start_plan", start_plan, plan, 8, true, true}};
    if (int rc = check_ops_given(ops, 3)) return rc;
    if (n_utt == 0) return B2H_OK;
    if (int rc = check_ops_memory(ops, 3, true)) return rc;
    EpArgs a;
    a.offsets = offsets; a.utt_plan = utt_plan; a.start_plan = start_plan;
    a.n_utt = n_utt; a.T = T;
    a.key0 = (uint32_t)seed; a.key1 = (uint32_t)(seed >> 32);
    a.epoch0 = (uint32_t)epoch; a.epoch1 = (uint32_t)(epoch >> 32);
    a.h = 1;
    while (((int64_t)1 << (2 * a.h)) < n_utt) ++a.h;
    a.shuffle = shuffle; a.random_crop = random_crop;
    const unsigned blocks = (unsigned)((n_utt + kEpThreads - 1) / kEpThreads);
    hipLaunchKernelGGL(b2h_epoch_plan_k, dim3(blocks), dim3(kEpThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

int b2h_epoch_record(const float* loss, float* losses, int64_t n_losses, int64_t* step, void* stream) {
    if (n_losses < 0) return fail(B2H_ERR_SHAPE, "negative shape");
    if (n_losses > ((int64_t)1 << 40)) return fail(B2H_ERR_SHAPE, "n_losses too large");
    if (!loss) return fail(B2H_ERR_INVALID, "loss is NULL");
    if (!losses && n_losses > 0) return fail(B2H_ERR_INVALID, "losses is NULL");
    if (!step) return fail(B2H_ERR_INVALID, "step is NULL");
    if (misaligned(loss, 4) || misaligned(losses, 4)) return fail(B2H_ERR_INVALID, "loss and losses must be 4-byte aligned");
    if (misaligned(step, 8)) return fail(B2H_ERR_INVALID, "step must be 8-byte aligned");
    const size_t bytes = (size_t)n_losses * 4;
    std::vector<Span> out_spans = {{step, 8}};
    if (bytes) out_spans.push_back({losses, bytes});
    if (int rc = check_overlap(out_spans, {{loss, 4, "loss"}})) return rc;
    if (int rc = check_device_ptr(loss, "loss")) return rc;
    if (bytes)
        if (int rc = check_device_ptr(losses, "losses")) return rc;
    if (int rc = check_device_ptr(step, "step")) return rc;
    hipLaunchKernelGGL(b2h_epoch_record_k, dim3(1), dim3(1), 0, (hipStream_t)stream, loss, losses, n_losses, step);
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

// ---- whole-store inference: the window plan, the row write-back, the joint error (kernel_scatter_rows.h) -------
int64_t b2h_window_plan(const int64_t* offsets, int64_t n_utt, int64_t T, int coverage, int64_t* utt_plan,
                        int64_t* start_plan, int64_t* skip_plan, int64_t capacity) {
    return window_plan(offsets, n_utt, T, coverage, 0, utt_plan, start_plan, skip_plan, capacity);
}

int64_t b2h_window_plan_overlap(const int64_t* offsets, int64_t n_utt, int64_t T, int64_t overlap, int64_t* utt_plan,
                                int64_t* start_plan, int64_t* skip_plan, int64_t capacity) {
    return window_plan(offsets, n_utt, T, B2H_COVER_ALL, overlap, utt_plan, start_plan, skip_plan, capacity);
}

int b2h_scatter_rows(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body,
                     const int64_t* utt, const int64_t* start, const int64_t* skip, int64_t B, int64_t T, int predict,
                     int flags, float factor, const float* pred, float conf, float* rows_out, void* stream) {
    return scatter_rows(rows, n_rows, offsets, n_utt, n_body, utt, start, skip, B, T, predict, flags, factor, pred, conf,
                        rows_out, stream);
}

int b2h_scatter_rows_blend(const float* rows, int64_t n_rows, const int64_t* offsets, int64_t n_utt, int n_body,
                           const int64_t* utt_plan, const int64_t* start_plan, const int64_t* skip_plan, int64_t n_plan,
                           int64_t entry0, int64_t B, int64_t T, int predict, int flags, float factor, const float* pred,
                           const float* pred_before, int blend, float conf, float* rows_out, void* stream) {
    const RowsBlend with = {n_plan, entry0, pred_before, blend};
    return scatter_rows(rows, n_rows, offsets, n_utt, n_body, utt_plan, start_plan, skip_plan, B, T, predict, flags, factor,
                        pred, conf, rows_out, stream, &with);
}

int b2h_joint_error(const float* rows_pred, const float* rows_true, int64_t n_rows, const int64_t* offsets, int64_t n_utt,
                    int n_body, float* utt_sum, int32_t* utt_count, double* total_sum, int64_t* total_count, void* stream) {
    if (n_rows < 0 || n_utt < 0) return fail(B2H_ERR_SHAPE, "negative shape");
    if (n_body != 8 && n_body != 12) return fail(B2H_ERR_INVALID, "n_body must be 8 or 12");
    if (!total_sum != !total_count) return fail(B2H_ERR_INVALID, "total_sum and total_count go together: both or neither");
    if (n_rows > ((int64_t)1 << 40) || n_utt > ((int64_t)1 << 30)) return fail(B2H_ERR_SHAPE, "store too large");
    if (n_utt == 0 && !total_sum) return B2H_OK;
    const size_t store = (size_t)n_rows * 3 * (n_body + 42) * 4, cells = (size_t)n_utt * kJeJoints;
    const Op ops[] = {{"rows_pred", rows_pred, store, 4, n_rows == 0, false},
                      {"rows_true", rows_true, store, 4, n_rows == 0, false},
                      {"offsets", offsets, (size_t)(n_utt + 1) * 8, 8, n_utt == 0, false},
                      {"utt_sum", utt_sum, cells * 4, 4, n_utt == 0, true},
                      {"utt_count", utt_count, cells * 4, 4, n_utt == 0, true},
                      {"total_sum", total_sum, kJeJoints * 8, 8, true, true},
                      {"total_count", total_count, kJeJoints * 8, 8, true, true}};
    if (int rc = check_ops(ops, false)) return rc;
    JeArgs a;
    a.rows_pred = rows_pred; a.rows_true = rows_true; a.offsets = offsets; a.utt_sum = utt_sum; a.utt_count = utt_count;
    a.total_sum = total_sum; a.total_count = total_count; a.n_rows = n_rows; a.n_utt = n_utt; a.n_body = n_body;
    if (n_utt > 0) {
        const unsigned blocks = (unsigned)((cells + kJeThreads - 1) / kJeThreads);
        hipLaunchKernelGGL(b2h_joint_error_k, dim3(blocks), dim3(kJeThreads), 0, (hipStream_t)stream, a);
        HIP_TRY(hipGetLastError());
    }
    if (total_sum) {
        hipLaunchKernelGGL(b2h_joint_total_k, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
        HIP_TRY(hipGetLastError());
    }
    return B2H_OK;
}

} // extern "C"

// ---- training (kernel_train.h) ------------------------------------------------------------------------------
namespace {
int odd_stride(int n) { return n | 1; }

TrainParams train_params(const b2h_model* m, const float* const* params) {
    TrainParams p;
    int off = 0; // < 2^18 floats at 128 channels
    for (int l = 0; l < 4; ++l) {
        p.w[l] = params[2 * l];
        p.b[l] = params[2 * l + 1];
        p.off[2 * l] = off;
        off += m->cout[l] * m->cin[l] * kTaps;
        p.off[2 * l + 1] = off;
        off += m->cout[l];
    }
    p.C = m->C;
    p.cin0 = m->cin[0];
    p.pos_emb = m->pos_emb;
    p.xs = odd_stride(m->cin[0]);
    p.as = odd_stride(m->C);
    p.gs = odd_stride(kOutCh);
    p.slab = (off + 3) / 4 * 4;
    return p;
}

int64_t train_param_floats(const TrainParams& p) { return p.off[7] + kOutCh; }

size_t train_lds_bytes(const TrainParams& p, int mode) {
    const int R = train_rows(mode);
    return (size_t)R * (p.xs + 3 * p.as + (mode ? p.gs : 0)) * 4;
}

// Tiles of a backward launch -> slabs: depends on (B, T) and the width only, never on the device.
int64_t train_tiles(int64_t B, int64_t T, int mode) { return B * ((T + train_tile(mode) - 1) / train_tile(mode)); }
int train_nslabs(const TrainParams& p, int64_t B, int64_t T) {
    // at most 2^26 floats (256 MiB) of slabs, at least 64 slabs
    const int64_t cap = std::max<int64_t>(64, std::min<int64_t>(kTrainMaxSlabs, ((int64_t)1 << 26) / p.slab));
    return (int)std::min<int64_t>(train_tiles(B, T, 1), cap);
}

int set_train_kernel_attributes() {
    static OncePerDevice once;
    return once([]() -> int {
        int rc;
        if ((rc = raise_lds_cap(b2h_train_conv<0>)) || (rc = raise_lds_cap(b2h_train_conv<1>)) ||
            (rc = raise_lds_cap(b2h_train_conv<2>)))
            return rc;
        return B2H_OK;
    });
}

// Shared checks of b2h_train_forward / b2h_backward, as launch() makes them for b2h_forward.
int train_check(const b2h_model* m, const float* const* params, int64_t B, int64_t T) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    if (int rc = check_shape(m, B, T)) return rc;
    if (!params) return fail(B2H_ERR_INVALID, "params is NULL");
    for (int i = 0; i < 8; ++i) {
        if (!params[i]) return fail(B2H_ERR_INVALID, "params[" + std::to_string(i) + "] is NULL");
        if (misaligned(params[i], 4)) return fail(B2H_ERR_INVALID, "params must be 4-byte aligned fp32 tensors");
    }
    return B2H_OK;
}

// Shape and device-pointer checks of the L1 metrics (grad = false: outputs a, b = per_seq, loss) and of their
// gradients (grad = true: a, b = dloss, dpred).
int l1_check(bool grad, const float* pred, const float* target, const float* scores, const int64_t* n_frames,
             int64_t B, int64_t T, int J, const float* a, const char* a_name, const float* b, const char* b_name) {
    if (J < 1 || J > 1024) return fail(B2H_ERR_SHAPE, "the L1 metrics take 1 <= n_joints <= 1024 joints per frame");
    if (B < 1 || T < 1)
        return grad ? fail(B2H_ERR_SHAPE, "the L1 loss gradients need B >= 1 and T >= 1")
                    : fail(B2H_ERR_SHAPE, "the L1 metrics need B >= 1 and T >= 1");
    if (B > 0x7fffffff || T > (1 << 24)) return fail(B2H_ERR_SHAPE, "shape too large");
    int rc;
    if ((rc = check_device_ptr(pred, "pred")) || (rc = check_device_ptr(target, "target")) ||
        (rc = check_device_ptr(a, a_name)) || (rc = check_device_ptr(b, b_name)) ||
        (scores && (rc = check_device_ptr(scores, "scores"))) || (n_frames && (rc = check_device_ptr(n_frames, "n_frames"))))
        return rc;
    return B2H_OK;
}

int l1_metric(const float* pred, const float* target, const float* scores, const int64_t* n_frames, int64_t B,
              int64_t T, int J, float* per_seq, float* loss, void* stream) {
    if (int rc = l1_check(false, pred, target, scores, n_frames, B, T, J, per_seq, "per_seq", loss, "loss")) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(scores ? b2h_masked_l1_seq_kernel<true> : b2h_masked_l1_seq_kernel<false>, dim3((unsigned)B),
                       dim3(256), 0, st, pred, target, scores, n_frames, per_seq, (int)T, 2 * J);
    hipLaunchKernelGGL(b2h_mean_kernel, dim3(1), dim3(256), 0, st, per_seq, loss, B, scores ? 0 : 1);
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

int l1_backward(const float* pred, const float* target, const float* scores, const int64_t* n_frames, int64_t B,
                int64_t T, int J, const float* dloss, float* dpred, void* stream) {
    if (int rc = l1_check(true, pred, target, scores, n_frames, B, T, J, dloss, "dloss", dpred, "dpred")) return rc;
    if (misaligned(pred, 16) || misaligned(target, 16) || misaligned(dpred, 16))
        return fail(B2H_ERR_INVALID, "pred, target and dpred must be 16-byte aligned");
    const size_t pn = (size_t)B * T * 2 * J * 4;
    if (overlaps(dpred, pn, pred, pn) || overlaps(dpred, pn, target, pn) || overlaps(dpred, pn, dloss, 4) ||
        (scores && overlaps(dpred, pn, scores, pn / 2)) || (n_frames && overlaps(dpred, pn, n_frames, (size_t)B * 8)))
        return fail(B2H_ERR_INVALID, "dpred overlaps an input");
    const int64_t n = B * T * J;
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 256 * 16);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(scores ? b2h_l1_backward_kernel<true> : b2h_l1_backward_kernel<false>, dim3((unsigned)blocks),
                       dim3(256), 0, st, pred, target, scores, n_frames, dloss, dpred, B, (int)T, 2 * J);
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}
} // namespace

extern "C" {

int b2h_version(void) { return B2H_VERSION; }
int b2h_build_flags(void) { return B2H_ABLATE; }

const char* b2h_last_error(void) { return g_err.c_str(); }

int b2h_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    return ok;
}

int b2h_create(int conv_channels, const char* activation, int pos_emb, b2h_model** out) {
    if (!out) return fail(B2H_ERR_INVALID, "out is NULL");
    *out = nullptr;
    // HandPoseModels.py:34-37: only "ReLU" is accepted, anything else raises ValueError
    if (!activation || std::strcmp(activation, "ReLU") != 0)
        return fail(B2H_ERR_INVALID, "activation must be \"ReLU\" (HandPoseModels.py:34-37)");
    if (conv_channels < 1 || conv_channels > kMaxWidth)
        return fail(B2H_ERR_INVALID, "conv_channels must be in [1, 128]");
    std::unique_ptr<b2h_model> m(new b2h_model()); // released to the caller only on success
    if (int rc = probe_device(m->device, m->num_cus)) return rc;
    m->C = conv_channels;
    m->pos_emb = pos_emb ? 1 : 0;
    const int C = conv_channels;
    const int cin[4] = {kInCh + m->pos_emb, C, C, C}, cout[4] = {C, C, C, kOutCh};
    for (int l = 0; l < 4; ++l) { m->cin[l] = cin[l]; m->cout[l] = cout[l]; }
    if (int rc = set_train_kernel_attributes()) return rc; // before any launch: the training entry points stay capturable
    *out = m.release();
    return B2H_OK;
}

int b2h_destroy(b2h_model* m) {
    delete m;
    return B2H_OK;
}

int b2h_load_weights(b2h_model* m, const float* w1, const float* b1, const float* w2, const float* b2,
                     const float* w3, const float* b3, const float* w4, const float* b4, int on_device) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    const float* tensors[8] = {w1, b1, w2, b2, w3, b3, w4, b4};
    std::vector<size_t> sizes;
    for (int l = 0; l < 4; ++l) {
        if (!tensors[2 * l] || !tensors[2 * l + 1]) return fail(B2H_ERR_INVALID, "weight pointer is NULL");
        sizes.push_back((size_t)m->cout[l] * m->cin[l] * kTaps);
        sizes.push_back(m->cout[l]);
    }
    std::vector<std::vector<float>> h;
    int rc;
    if ((rc = fetch_tensors(tensors, sizes, on_device, h)) || (rc = check_device(m->device))) return rc;
    HostWeights hw;
    hw.m = m;
    for (int l = 0; l < 4; ++l) {
        hw.w[l] = std::move(h[2 * l]);
        hw.b[l] = std::move(h[2 * l + 1]);
    }
    if ((rc = set_conv_kernel_attributes())) return rc;
    if ((rc = pack_all(m, hw))) return rc;
    m->has_weights = true;
    return B2H_OK;
}

int b2h_forward(b2h_model* m, const float* x, float* y, int64_t B, int64_t T, int kernel, void* stream) {
    FusedArgs fa{0, 1.0f, nullptr};
    return launch(m, x, y, B, T, kernel, fa, (hipStream_t)stream);
}

int b2h_forward_fused(b2h_model* m, const float* body, float* y, int64_t B, int64_t T, int flags, float factor,
                      const int64_t* n_frames, int kernel, void* stream) {
    if (int rc = check_fused(flags, factor)) return rc;
    FusedArgs fa{flags, factor, n_frames};
    return launch(m, body, y, B, T, kernel, fa, (hipStream_t)stream);
}

int b2h_target_transform(const float* body, const float* hand, float* hand_out, int64_t B, int64_t T, int flags,
                         float factor, void* stream) {
    if (B < 0 || T < 0) return fail(B2H_ERR_SHAPE, "negative shape");
    if (B * T == 0) return B2H_OK;
    if (B > 0x7fffffff || T > (1 << 24)) return fail(B2H_ERR_SHAPE, "shape too large");
    if (flags & ~3) return fail(B2H_ERR_INVALID, "unknown flag bits");
    if ((flags & 2) && !(factor > 0.f)) return fail(B2H_ERR_INVALID, "factor must be > 0");
    int rc;
    if ((rc = check_device_ptr(body, "body")) || (rc = check_device_ptr(hand, "hand")) ||
        (rc = check_device_ptr(hand_out, "hand_out")))
        return rc;
    const int64_t n = B * T * 21;
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 256 * 8);
    hipLaunchKernelGGL(b2h_target_transform_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, body,
                       hand, hand_out, B * T, flags, factor);
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

int b2h_masked_l1_joints(const float* pred, const float* target, const int64_t* n_frames, int64_t B, int64_t T,
                         int n_joints, float* per_seq, float* loss, void* stream) {
    return l1_metric(pred, target, nullptr, n_frames, B, T, n_joints, per_seq, loss, stream);
}

int b2h_weighted_l1_joints(const float* pred, const float* target, const float* scores, const int64_t* n_frames, int64_t B,
                           int64_t T, int n_joints, float* per_seq, float* loss, void* stream) {
    if (!scores) return fail(B2H_ERR_INVALID, "scores is NULL");
    return l1_metric(pred, target, scores, n_frames, B, T, n_joints, per_seq, loss, stream);
}

int b2h_masked_l1_joints_backward(const float* pred, const float* target, const int64_t* n_frames, int64_t B, int64_t T,
                                  int n_joints, const float* dloss, float* dpred, void* stream) {
    return l1_backward(pred, target, nullptr, n_frames, B, T, n_joints, dloss, dpred, stream);
}

int b2h_weighted_l1_joints_backward(const float* pred, const float* target, const float* scores, const int64_t* n_frames,
                                    int64_t B, int64_t T, int n_joints, const float* dloss, float* dpred, void* stream) {
    if (!scores) return fail(B2H_ERR_INVALID, "scores is NULL");
    return l1_backward(pred, target, scores, n_frames, B, T, n_joints, dloss, dpred, stream);
}

int b2h_masked_l1(const float* pred, const float* target, const int64_t* n_frames, int64_t B, int64_t T,
                  float* per_seq, float* loss, void* stream) {
    return b2h_masked_l1_joints(pred, target, n_frames, B, T, kOutCh / 2, per_seq, loss, stream);
}

int b2h_weighted_l1(const float* pred, const float* target, const float* scores, const int64_t* n_frames, int64_t B,
                    int64_t T, float* per_seq, float* loss, void* stream) {
    return b2h_weighted_l1_joints(pred, target, scores, n_frames, B, T, kOutCh / 2, per_seq, loss, stream);
}

int b2h_train_forward(b2h_model* m, const float* const* params, const float* x, float* y, int64_t B, int64_t T,
                      void* stream) {
    if (int rc = train_check(m, params, B, T)) return rc;
    if (B == 0) return B2H_OK;
    if (int rc = check_xy(m, x, y, B, T)) return rc;
    const size_t yn = (size_t)B * T * kOutCh * 4;
    for (int i = 0; i < 8; ++i)
        if (overlaps(params[i], 4, y, yn)) return fail(B2H_ERR_INVALID, "y overlaps a parameter");
    const TrainParams p = train_params(m, params);
    const int64_t tiles = train_tiles(B, T, 0);
    if (tiles > 0x7fffffff) return fail(B2H_ERR_SHAPE, "B*T too large for one launch");
    const int tps = (int)((T + kTrainFwdTile - 1) / kTrainFwdTile);
    hipLaunchKernelGGL(b2h_train_conv<0>, dim3((unsigned)tiles), dim3(256), train_lds_bytes(p, 0), (hipStream_t)stream,
                       x, nullptr, y, nullptr, p, (int)T, tps, tiles, 0);
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

size_t b2h_backward_workspace_bytes(const b2h_model* m, int64_t B, int64_t T) {
    if (!m || B < 1 || T < 1) return 0;
    float* dummy[8] = {};
    const TrainParams p = train_params(m, dummy);
    return (size_t)train_nslabs(p, B, T) * p.slab * 4;
}

int b2h_backward(b2h_model* m, const float* const* params, const float* x, const float* dy, float* dx,
                 float* const* grads, int64_t B, int64_t T, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = train_check(m, params, B, T)) return rc;
    if (B == 0) return fail(B2H_ERR_SHAPE, "b2h_backward needs B >= 1 (the gradients of an empty batch are not defined here)");
    if (!x || !dy) return fail(B2H_ERR_INVALID, "x / dy is NULL");
    if (!grads) return fail(B2H_ERR_INVALID, "grads is NULL");
    if (int rc = check_device(m->device)) return rc;
    if (misaligned(x, 16) || misaligned(dy, 16) || (dx && misaligned(dx, 16)) || misaligned(workspace, 16))
        return fail(B2H_ERR_INVALID, "x, dy, dx and the workspace must be 16-byte aligned");
    const TrainParams p = train_params(m, params);
    const int nslabs = train_nslabs(p, B, T);
    const size_t need = (size_t)nslabs * p.slab * 4;
    if (!workspace || workspace_bytes < need)
        return fail(B2H_ERR_INVALID, "workspace smaller than b2h_backward_workspace_bytes (" + std::to_string(need) + " B)");
    const size_t xn = (size_t)B * T * kInCh * 4, yn = (size_t)B * T * kOutCh * 4;
    auto param_bytes = [&](int i) { return (size_t)((i + 1 < 8 ? p.off[i + 1] : train_param_floats(p)) - p.off[i]) * 4; };
    // outputs: the eight gradients, dx, the workspace; none may overlap another operand
    std::vector<Span> outs, read_only = {{x, xn, "x or dy"}, {dy, yn, "x or dy"}};
    for (int i = 0; i < 8; ++i) {
        if (!grads[i]) return fail(B2H_ERR_INVALID, "grads[" + std::to_string(i) + "] is NULL");
        if (misaligned(grads[i], 4)) return fail(B2H_ERR_INVALID, "grads must be 4-byte aligned");
        outs.push_back({grads[i], param_bytes(i)});
        read_only.push_back({params[i], param_bytes(i), "a parameter"});
    }
    if (dx) outs.push_back({dx, xn});
    outs.push_back({workspace, need});
    if (int rc = check_overlap(outs, read_only)) return rc;
    const int64_t tiles = train_tiles(B, T, 1);
    const int tps = (int)((T + kTrainBwdTile - 1) / kTrainBwdTile);
    hipStream_t st = (hipStream_t)stream;
    float* ws = static_cast<float*>(workspace);
    hipLaunchKernelGGL(dx ? b2h_train_conv<2> : b2h_train_conv<1>, dim3((unsigned)nslabs), dim3(256),
                       train_lds_bytes(p, dx ? 2 : 1), st, x, dy, dx, ws, p, (int)T, tps, tiles, nslabs);
    TrainGrads g;
    for (int i = 0; i < 8; ++i) {
        g.g[i] = grads[i];
        g.off[i] = p.off[i];
    }
    g.off[8] = train_param_floats(p);
    hipLaunchKernelGGL(b2h_train_reduce, dim3((unsigned)((g.off[8] + 63) / 64)), dim3(256), 0, st, ws, p.slab, nslabs, g);
    HIP_TRY(hipGetLastError());
    return B2H_OK;
}

int b2h_masked_l1_backward(const float* pred, const float* target, const int64_t* n_frames, int64_t B, int64_t T,
                           const float* dloss, float* dpred, void* stream) {
    return b2h_masked_l1_joints_backward(pred, target, n_frames, B, T, kOutCh / 2, dloss, dpred, stream);
}

int b2h_weighted_l1_backward(const float* pred, const float* target, const float* scores, const int64_t* n_frames,
                             int64_t B, int64_t T, const float* dloss, float* dpred, void* stream) {
    if (!scores) return fail(B2H_ERR_INVALID, "scores is NULL");
    return b2h_weighted_l1_joints_backward(pred, target, scores, n_frames, B, T, kOutCh / 2, dloss, dpred, stream);
}

int b2h_model_info(const b2h_model* m, int* conv_channels, int* pos_emb, int* has_weights) {
    if (!m) return fail(B2H_ERR_INVALID, "model is NULL");
    if (conv_channels) *conv_channels = m->C;
    if (pos_emb) *pos_emb = m->pos_emb;
    if (has_weights) *has_weights = m->has_weights ? 1 : 0;
    return B2H_OK;
}

int b2h_kernel_supported(const b2h_model* m, int kernel) {
    if (!m) return 0;
    return kernel_ok(m, resolve_kernel(m, kernel)) ? 1 : 0;
}

const char* b2h_kernel_name(const b2h_model* m, int kernel) {
    if (!m) return "";
    const int k = resolve_kernel(m, kernel);
    if (const ChunkVariant* v = chunk_variant(k, m->C > kMfmaWidth)) return v->name;
    switch (k) { // the persistent kernel is named by its streaming instantiation
        case B2H_KERNEL_F32_VALU: return "b2h_fwd_f32_valu";
        case B2H_KERNEL_BF16_MFMA: return "b2h_fwd_mfma16<1, false, true>";
        case B2H_KERNEL_F16_MFMA: return "b2h_fwd_mfma16<2, false, true>";
        default: return "";
    }
}

int b2h_time_forward(b2h_model* m, const float* x, float* y, int64_t B, int64_t T, int kernel, int iters,
                     void* stream, float* avg_ms) {
    if (iters < 1 || !avg_ms) return fail(B2H_ERR_INVALID, "iters < 1 or avg_ms NULL");
    hipStream_t st = (hipStream_t)stream;
    Event e0, e1;
    HIP_TRY(hipEventCreate(&e0.e));
    HIP_TRY(hipEventCreate(&e1.e));
    FusedArgs fa{0, 1.0f, nullptr};
    int rc = B2H_OK;
    HIP_TRY(hipEventRecord(e0.e, st));
    for (int i = 0; i < iters && rc == B2H_OK; ++i) rc = launch(m, x, y, B, T, kernel, fa, st);
    HIP_TRY(hipEventRecord(e1.e, st));
    HIP_TRY(hipEventSynchronize(e1.e));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0.e, e1.e));
    if (rc) return rc;
    *avg_ms = ms / iters;
    return B2H_OK;
}

int b2h_stream_sync(void* stream) {
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return B2H_OK;
}

} // extern "C"

#include "dev/b2h_dev_exports.h" // empty unless a B2H_ABLATE stamp build
