// GF(2^8) region engine, host tier: the 3-slot pipeline for host-resident batches (engine.hpp run_host_pipeline).
#include <condition_variable>
#include <thread>

#include "engine_internal.hpp"

namespace ecg {

// Page-locked (hipHostMalloc'd or registered) host memory, as opposed to ordinary pageable memory.
static bool host_pinned(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

int Engine::run_host_pipeline(const LinearOp& prog, const void* h_in, long long in_sstride, long long in_bstride,
                              void* h_out, long long out_sstride, long long out_bstride, long long B, int S,
                              int chunk) {
    if (S < 0 || B < 0 || prog.k_in() < 1 || prog.m_out() < 1) return ECG_EINVAL;
    if (S == 0 || B == 0) return ECG_OK;
    if (!h_in || !h_out) return ECG_EINVAL;
    if (const int rc = batch_flush_pending(); rc != ECG_OK) return rc;
    if (chunk < 1) chunk = 16;
    if (chunk > S) chunk = S;
    const int kin = prog.k_in(), mout = prog.m_out();
    const size_t pitch = ((size_t)B + 255) & ~(size_t)255;
    const size_t slot_in = (size_t)chunk * kin * pitch, slot_out = (size_t)chunk * mout * pitch;
    CtxLease lease(device_);
    HostCtx& c = *lease;
    if (!c.pipe_ready) {
        for (int i = 0; i < 3; i++) {
            ECG_HIP(hipStreamCreateWithFlags(&c.pstream[i], hipStreamNonBlocking));
            ECG_HIP(hipEventCreateWithFlags(&c.in_done[i], hipEventDisableTiming));
            ECG_HIP(hipEventCreateWithFlags(&c.comp_done[i], hipEventDisableTiming));
            ECG_HIP(hipEventCreateWithFlags(&c.out_done[i], hipEventDisableTiming));
        }
        c.pipe_ready = true;
    }
    if (c.pslot_cap < 3 * (slot_in + slot_out)) {
        for (int i = 0; i < 3; i++) ECG_HIP(hipStreamSynchronize(c.pstream[i]));
        if (c.pslot) (void)hipFree(c.pslot);
        c.pslot = nullptr;
        c.pslot_cap = 0;
        ECG_HIP(hipMalloc(&c.pslot, 3 * (slot_in + slot_out)));
        c.pslot_cap = 3 * (slot_in + slot_out);
    }
    // the device program reads compact slot blocks 0..kin-1 and writes 0..mout-1
    LinearOp dev = prog;
    for (int j = 0; j < kin; j++) dev.src_ids[j] = j;
    for (int p = 0; p < mout; p++) dev.dst_ids[p] = p;
    int status = ECG_OK;
    hipStream_t s_in = c.pstream[0], s_comp = c.pstream[1], s_out = c.pstream[2];
    std::shared_ptr<ProgramSet> ps = program_set(&dev, 1, &status, s_comp);
    if (!ps) return status;
    if (const int rc = ps->ensure_ready(s_comp); rc != ECG_OK) return rc;
    const uint8_t* hin = (const uint8_t*)h_in;
    uint8_t* hout = (uint8_t*)h_out;
    const bool in_pinned = host_pinned(h_in), out_pinned = host_pinned(h_out);
    const int nchunks = (int)((S + (long long)chunk - 1) / chunk);
    auto issue_out = [&](int it) -> int {  // D2H of chunk it, behind its kernel
        const int s0 = it * chunk, n = std::min(chunk, S - s0), slot = it % 3;
        uint8_t* dout = c.pslot + (size_t)slot * (slot_in + slot_out) + slot_in;
        ECG_HIP(hipStreamWaitEvent(s_out, c.comp_done[slot], 0));
        for (int p = 0; p < mout; p++)
            ECG_HIP(hipMemcpy2DAsync(hout + (size_t)s0 * out_sstride + (size_t)prog.dst_ids[p] * out_bstride,
                                     (size_t)out_sstride, dout + (size_t)p * pitch, (size_t)mout * pitch, (size_t)B,
                                     (size_t)n, hipMemcpyDeviceToHost, s_out));
        ECG_HIP(hipEventRecord(c.out_done[slot], s_out));
        return ECG_OK;
    };
    // A copy to or from pageable memory (the proxy's own vectors) returns only once the runtime has moved
    // the bytes, so issued from one thread the input and output copies of a pageable batch run one after
    // the other: RS(10,4) 1 MiB encode 36 GiB/s of data, the H2D and D2H times added.  PCIe is full
    // duplex: with either side pageable, a second host thread issues the output copies (50 GiB/s, the
    // pinned rate; profiles/r02/pipeline/).  Copying pageable runs of consecutive blocks as 1-D copies,
    // which the runtime pins per copy above 1 MiB, measured slower than these 2-D copies and was dropped.
    // Chunk it's copies wait (host side) for its kernel to be enqueued; the kernel that reuses a slot waits
    // until the copies that drain it are enqueued, so every event wait refers to the intended record.
    struct OutThread {
        std::mutex mu;
        std::condition_variable cv;
        int comp_issued = 0, out_issued = 0, rc = ECG_OK;
        std::string msg;  // the copy thread's error message (last_error is per thread)
        bool stop = false;
        std::thread th;
        void finish() {
            if (!th.joinable()) return;
            {
                std::lock_guard<std::mutex> lk(mu);
                stop = true;
            }
            cv.notify_all();
            th.join();
        }
        ~OutThread() { finish(); }
    } ot;
    const bool split = !in_pinned || !out_pinned;
    if (split) {
        ot.th = std::thread([&] {
            if (hipSetDevice(device_) != hipSuccess) {  // the current device is per host thread
                std::lock_guard<std::mutex> lk(ot.mu);
                ot.rc = ECG_EHIP;
                ot.msg = "host pipeline: hipSetDevice failed on the copy thread";
                ot.cv.notify_all();
                return;
            }
            for (int it = 0; it < nchunks; it++) {
                {
                    std::unique_lock<std::mutex> lk(ot.mu);
                    ot.cv.wait(lk, [&] { return ot.comp_issued > it || ot.stop; });
                    if (ot.comp_issued <= it) return;  // stopped early (error on the issuing thread)
                }
                const int rc = issue_out(it);
                {
                    std::lock_guard<std::mutex> lk(ot.mu);
                    if (rc != ECG_OK) {
                        ot.rc = rc;
                        ot.msg = last_error_string();
                    } else {
                        ot.out_issued = it + 1;
                    }
                }
                ot.cv.notify_all();
                if (rc != ECG_OK) return;
            }
        });
    }
    for (int it = 0; it < nchunks; it++) {
        const int s0 = it * chunk, n = std::min(chunk, S - s0), slot = it % 3;
        const bool reuse = it >= 3;
        uint8_t* din = c.pslot + (size_t)slot * (slot_in + slot_out);
        uint8_t* dout = din + slot_in;
        if (reuse) ECG_HIP(hipStreamWaitEvent(s_in, c.comp_done[slot], 0));  // slot's inputs consumed
        for (int j = 0; j < kin; j++)
            ECG_HIP(hipMemcpy2DAsync(din + (size_t)j * pitch, (size_t)kin * pitch,
                                     hin + (size_t)s0 * in_sstride + (size_t)prog.src_ids[j] * in_bstride,
                                     (size_t)in_sstride, (size_t)B, (size_t)n, hipMemcpyHostToDevice, s_in));
        ECG_HIP(hipEventRecord(c.in_done[slot], s_in));
        ECG_HIP(hipStreamWaitEvent(s_comp, c.in_done[slot], 0));
        if (reuse) {
            if (split) {  // the copies draining this slot (chunk it - 3) must be enqueued first
                std::unique_lock<std::mutex> lk(ot.mu);
                ot.cv.wait(lk, [&] { return ot.out_issued >= it - 2 || ot.rc != ECG_OK; });
                if (ot.rc != ECG_OK) {
                    set_last_error(ot.msg);
                    return ot.rc;
                }
            }
            ECG_HIP(hipStreamWaitEvent(s_comp, c.out_done[slot], 0));  // slot's outputs copied out
        }
        GfLaunch a = launch_args(*ps, B, n);
        a.in_base = din;
        a.out_base = dout;
        a.in_sstride = (long long)(kin * pitch);
        a.in_bstride = (long long)pitch;
        a.out_sstride = (long long)(mout * pitch);
        a.out_bstride = (long long)pitch;
        ECG_HIP(launch_gf(a, GF_MODE_STRIDED, true, s_comp));
        ECG_HIP(hipEventRecord(c.comp_done[slot], s_comp));
        if (split) {
            {
                std::lock_guard<std::mutex> lk(ot.mu);
                ot.comp_issued = it + 1;
            }
            ot.cv.notify_all();
        } else if (const int rc = issue_out(it); rc != ECG_OK) {
            return rc;
        }
    }
    if (split) {
        ot.th.join();
        if (ot.rc != ECG_OK) {
            set_last_error(ot.msg);
            return ot.rc;
        }
    }
    ECG_HIP(hipStreamSynchronize(s_out));
    return lease.done();
}

}  // namespace ecg
