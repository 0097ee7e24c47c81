// Pure C++/HIP host program that TRAINS over the C ABI (include/b2h.h): no Python, no torch.  The loop body of the
// reference (steps/traintest.py:105-121) for ConvModel with maskedPoseL1 and Adam:
//   b2h_train_forward -> tail mask -> b2h_masked_l1 -> b2h_masked_l1_backward -> b2h_backward -> b2h_adam_step
// all on one stream, nothing read back until the last step has been queued.
//
//   c_abi_train_host <in.bin> <out.bin>
//     in.bin : int32 C, pos_emb, B, T, steps; float32 lr; w1 b1 w2 b2 w3 b3 w4 b4 (fp32, reference state_dict
//              layout); x (B,T,12,2) fp32; target (B,T,21,2) fp32; lengths (B) int64
//     out.bin: the loss of every step (steps fp32, each taken before that step's update), then the eight updated tensors
//
//   hipcc -O2 --offload-arch=gfx950 -Iinclude -o c_abi_train_host examples/c_abi_train_host.cpp \
//         -Lhand_pose_sl_amd/csrc -lb2h -Wl,-rpath,$PWD/hand_pose_sl_amd/csrc
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "b2h.h"

#define CK(call)                                                                  \
    do {                                                                          \
        int rc_ = (call);                                                         \
        if (rc_ != B2H_OK) { std::fprintf(stderr, "%s -> %d: %s\n", #call, rc_, b2h_last_error()); return 2; } \
    } while (0)
#define HK(call)                                                                  \
    do {                                                                          \
        hipError_t e_ = (call);                                                   \
        if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 3; } \
    } while (0)

static bool read_all(FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 1; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 1; }
    int hdr[5];
    float lr;
    if (!read_all(f, hdr, sizeof hdr) || !read_all(f, &lr, 4)) return 1;
    const int C = hdr[0], pos_emb = hdr[1], B = hdr[2], T = hdr[3], steps = hdr[4], cin1 = 24 + (pos_emb ? 1 : 0);
    if (C < 1 || B < 1 || T < 1 || steps < 0) { std::fprintf(stderr, "bad header\n"); return 1; }
    const int64_t nw[8] = {(int64_t)C * cin1 * 5, C, (int64_t)C * C * 5, C, (int64_t)C * C * 5, C, (int64_t)42 * C * 5, 42};
    std::vector<std::vector<float>> w(8);
    for (int i = 0; i < 8; ++i) { w[i].resize(nw[i]); if (!read_all(f, w[i].data(), nw[i] * 4)) return 1; }
    std::vector<float> x((size_t)B * T * 24), target((size_t)B * T * 42);
    std::vector<int64_t> lengths(B);
    if (!read_all(f, x.data(), x.size() * 4) || !read_all(f, target.data(), target.size() * 4) ||
        !read_all(f, lengths.data(), (size_t)B * 8))
        return 1;
    std::fclose(f);

    if (b2h_version() != B2H_VERSION) { std::fprintf(stderr, "header/library version mismatch\n"); return 1; }
    if (b2h_device_count() < 1) { std::fprintf(stderr, "no gfx950 device\n"); return 4; }
    b2h_model* m = nullptr;
    CK(b2h_create(C, "ReLU", pos_emb, &m));
    hipStream_t st;
    HK(hipStreamCreate(&st));

    // parameters, gradients and the two Adam moments (zeros), one allocation each
    float *param[8], *grad[8], *avg[8], *avg_sq[8];
    for (int i = 0; i < 8; ++i) {
        HK(hipMalloc(&param[i], nw[i] * 4));
        HK(hipMalloc(&grad[i], nw[i] * 4));
        HK(hipMalloc(&avg[i], nw[i] * 4));
        HK(hipMalloc(&avg_sq[i], nw[i] * 4));
        HK(hipMemcpyAsync(param[i], w[i].data(), nw[i] * 4, hipMemcpyHostToDevice, st));
        HK(hipMemsetAsync(avg[i], 0, nw[i] * 4, st));
        HK(hipMemsetAsync(avg_sq[i], 0, nw[i] * 4, st));
    }
    float *dx, *dtarget, *dy, *dgrad_y, *per_seq, *losses, *one;
    int64_t* dlengths;
    void* ws;
    const size_t ws_bytes = b2h_backward_workspace_bytes(m, B, T);
    const float one_host = 1.f;
    HK(hipMalloc(&dx, x.size() * 4));
    HK(hipMalloc(&dtarget, target.size() * 4));
    HK(hipMalloc(&dy, target.size() * 4));
    HK(hipMalloc(&dgrad_y, target.size() * 4));
    HK(hipMalloc(&per_seq, (size_t)B * 4));
    HK(hipMalloc(&losses, (size_t)(steps + 1) * 4));
    HK(hipMalloc(&one, 4));
    HK(hipMalloc(&dlengths, (size_t)B * 8));
    HK(hipMalloc(&ws, ws_bytes ? ws_bytes : 16));
    HK(hipMemcpyAsync(dx, x.data(), x.size() * 4, hipMemcpyHostToDevice, st));
    HK(hipMemcpyAsync(dtarget, target.data(), target.size() * 4, hipMemcpyHostToDevice, st));
    HK(hipMemcpyAsync(dlengths, lengths.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
    HK(hipMemcpyAsync(one, &one_host, 4, hipMemcpyHostToDevice, st));

    for (int s = 0; s < steps; ++s) {
        CK(b2h_train_forward(m, param, dx, dy, B, T, st));                                   // prediction = model(x)
        for (int i = 0; i < B; ++i) {                                                        // mask_output: zero tails
            const int64_t n = lengths[i] < 0 ? 0 : (lengths[i] > T ? T : lengths[i]);
            if (n < T) HK(hipMemsetAsync(dy + ((size_t)i * T + n) * 42, 0, (size_t)(T - n) * 42 * 4, st));
        }
        CK(b2h_masked_l1(dy, dtarget, dlengths, B, T, per_seq, losses + s, st));             // loss = criterion(...)
        CK(b2h_masked_l1_backward(dy, dtarget, dlengths, B, T, one, dgrad_y, st));           // loss.backward()
        CK(b2h_backward(m, param, dx, dgrad_y, nullptr, grad, B, T, ws, ws_bytes, st));
        CK(b2h_adam_step(param, grad, avg, avg_sq, nw, 8, lr, nullptr, 0.9f, 0.999f, 1e-8f, 0.f, s + 1, nullptr,
                         st));                                                               // optimizer.step()
    }

    std::vector<float> host_losses(steps);
    if (steps) HK(hipMemcpyAsync(host_losses.data(), losses, (size_t)steps * 4, hipMemcpyDeviceToHost, st));
    for (int i = 0; i < 8; ++i) HK(hipMemcpyAsync(w[i].data(), param[i], nw[i] * 4, hipMemcpyDeviceToHost, st));
    CK(b2h_stream_sync(st));
    std::printf("trained %d steps  C=%d B=%d T=%d  last loss %g\n", steps, C, B, T, steps ? host_losses[steps - 1] : 0.f);

    CK(b2h_destroy(m));
    for (int i = 0; i < 8; ++i) { HK(hipFree(param[i])); HK(hipFree(grad[i])); HK(hipFree(avg[i])); HK(hipFree(avg_sq[i])); }
    HK(hipFree(dx)); HK(hipFree(dtarget)); HK(hipFree(dy)); HK(hipFree(dgrad_y)); HK(hipFree(per_seq)); HK(hipFree(losses));
    HK(hipFree(one)); HK(hipFree(dlengths)); HK(hipFree(ws)); HK(hipStreamDestroy(st));

    FILE* o = std::fopen(argv[2], "wb");
    if (!o || std::fwrite(host_losses.data(), 4, host_losses.size(), o) != host_losses.size()) return 1;
    for (int i = 0; i < 8; ++i)
        if (std::fwrite(w[i].data(), 4, w[i].size(), o) != w[i].size()) return 1;
    if (std::fclose(o) != 0) return 1;
    return 0;
}
