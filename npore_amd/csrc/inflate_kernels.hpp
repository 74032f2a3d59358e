// inflate_kernels.hpp -- BGZF in on the device: inflate_blocks_kernel runs inflate_wave.hpp's decoder, one wave per raw
// DEFLATE stream, and DeviceInflater puts it behind the window source of the one-pass BAM reader (bam_reader.hpp
// BamWindowSource) as its inflate hook -- the counterpart of bam_deflate_kernels.hpp on the input side.
//
// A workgroup is IW_WAVES_PER_GROUP = 4 waves, each with its own IwTables in LDS (3 676 bytes a wave, 14 704 a workgroup:
// eight workgroups, 32 waves, share a CU's 160 KiB), each with its own stream; the waves of a workgroup never wait for each
// other (no barrier).  A stream count that is no multiple of four leaves the last workgroup's spare waves idle.
//
// DeviceInflater::inflate_range has bgzf_inflate_range's signature (hostio.hpp) and does, for the blocks [b0, b1) of a window:
//   1. pread of the window's compressed bytes (payloads and trailers, one stretch of the file) into page-locked memory,
//      in pieces on the host's threads
//   2. one copy up, with the table of the blocks (where each payload lies, where its bytes go)
//   3. ONE launch for the window's non-empty blocks, timed by a pair of events
//   4. one copy of the inflated window down into the window's buffer
//   5. on the host's threads: the CRC-32 of every block's bytes against its trailer (unless NPORE_BGZF_CRC=0) -- in
//      production also the end-to-end check of what the device wrote --, and the host decoder (inflate_blocks) for every
//      block the device declined or whose bytes fail the CRC; the window fails only if that fails too
// on a stream of its own, from the reader's inflater thread (which selects the device itself); the buffers live as long
// as the inflater, that is for one run.  It assumes nothing about the size of a window.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <vector>

#include "devbuf.hpp"
#include "hostio.hpp"
#include "inflate_wave.hpp"

namespace npore {

constexpr int IW_WAVES_PER_GROUP = 4;

// stream k of n: in + in_off[k], in_len[k] bytes, must inflate to out_len[k] bytes at out + out_off[k] (the caller has
// checked that both ranges lie in their buffers); status[k] = 1 inflated, 0 declined or malformed
__global__ __launch_bounds__(64 * IW_WAVES_PER_GROUP) __attribute__((amdgpu_waves_per_eu(8, 8))) void inflate_blocks_kernel(const uint8_t *in, const int64_t *in_off, const int64_t *in_len,
                                                                                 uint8_t *out, const int64_t *out_off, const int64_t *out_len,
                                                                                 int64_t n, int32_t *status)
{
    __shared__ IwTables tables[IW_WAVES_PER_GROUP];
    const uint32_t wave = iw_uni(threadIdx.x >> 6);
    const int64_t k = (int64_t)blockIdx.x * IW_WAVES_PER_GROUP + wave;
    if (k >= n) return;
    const int64_t il = in_len[k], ol = out_len[k];
    int st = 0;
    if (il >= 0 && il <= (int64_t)IW_MAX_IN && ol >= 0 && ol <= (int64_t)IW_MAX_OUT) {
        InflateWave w(in + in_off[k], iw_uni((uint32_t)il), out + out_off[k], iw_uni((uint32_t)ol), tables[wave]);
        st = w.run();
    }
    if ((threadIdx.x & 63u) == 0u) status[k] = st;
}

inline void launch_inflate_blocks(const uint8_t *in, const int64_t *in_off, const int64_t *in_len, uint8_t *out, const int64_t *out_off,
                                  const int64_t *out_len, int64_t n, int32_t *status, hipStream_t s)
{
    if (n <= 0) return;
    const unsigned groups = (unsigned)((n + IW_WAVES_PER_GROUP - 1) / IW_WAVES_PER_GROUP);
    hipLaunchKernelGGL(inflate_blocks_kernel, dim3(groups), dim3(64 * IW_WAVES_PER_GROUP), 0, s, in, in_off, in_len, out, out_off, out_len, n, status);
}

// what npore_bam_inflate_info reports
enum { INFL_DEVICE = 0, INFL_DECLINED, INFL_CRC_FAILED, INFL_LAUNCHES, INFL_KERNEL_NS, INFL_BYTES_UP, INFL_BYTES_DOWN, INFL_INSTALLED, INFL_N };

class DeviceInflater {
public:
    explicit DeviceInflater(int device) : device_(device) {}
    DeviceInflater(const DeviceInflater &) = delete;
    DeviceInflater &operator=(const DeviceInflater &) = delete;
    ~DeviceInflater()
    {
        if (!s_) return;
        (void)hipSetDevice(device_);
        (void)hipStreamSynchronize(s_);
        (void)hipEventDestroy(e0_);
        (void)hipEventDestroy(e1_);
        (void)hipStreamDestroy(s_);
    }
    BgzfInflateFn hook()
    {
        return [this](const PreadFile &f, const std::vector<BgzfBlock> &blocks, size_t b0, size_t b1, uint8_t *dst, int threads) {
            return inflate_range(f, blocks, b0, b1, dst, threads) == NPORE_OK;
        };
    }
    void info(int64_t *out8) const
    {
        for (int k = 0; k < INFL_N; k++) out8[k] = n_[k].load();
        out8[INFL_INSTALLED] = 1;
    }
    // blocks [b0, b1) back to back into dst: NPORE_OK, or the code fail() returned (the words are this thread's)
    int inflate_range(const PreadFile &f, const std::vector<BgzfBlock> &blocks, size_t b0, size_t b1, uint8_t *dst, int threads)
    {
        if (b0 >= b1) return NPORE_OK;
        HIP_TRY(hipSetDevice(device_));
        if (!s_) {
            HIP_TRY(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
            HIP_TRY(hipEventCreate(&e0_));
            HIP_TRY(hipEventCreate(&e1_));
        }
        const uint64_t in0 = blocks[b0].in_off, in1 = blocks[b1 - 1].in_off + blocks[b1 - 1].in_len + 8;     // (+ 8: the last trailer)
        const uint64_t o0 = blocks[b0].out_off, o1 = blocks[b1 - 1].out_off + blocks[b1 - 1].out_len;
        const size_t comp_bytes = (size_t)(in1 - in0), out_bytes = (size_t)(o1 - o0);
        // the table: in_off | in_len | out_off | out_len of the non-empty blocks (an empty one has nothing to inflate)
        which_.clear();
        for (size_t i = b0; i < b1; i++) {
            const BgzfBlock &bk = blocks[i];
            if (bk.out_len > IW_MAX_OUT || bk.in_off < in0 || bk.in_off + bk.in_len + 8 > in1 || bk.out_off < o0 || bk.out_off + bk.out_len > o1)
                return fail(NPORE_E_INVALID, "corrupt BGZF block table");
            if (bk.out_len) which_.push_back(i);
        }
        const size_t n = which_.size();
        if (int rc = h_comp_.ensure(comp_bytes + 64)) return rc;
        if (int rc = h_meta_.ensure((n + 1) * 36)) return rc;
        if (int rc = d_comp_.ensure(comp_bytes + 64)) return rc;
        if (int rc = d_meta_.ensure((n + 1) * 36)) return rc;
        if (int rc = d_out_.ensure(out_bytes + 64)) return rc;
        int64_t *const m = h_meta_.as<int64_t>();
        for (size_t j = 0; j < n; j++) {
            const BgzfBlock &bk = blocks[which_[j]];
            m[j] = (int64_t)(bk.in_off - in0);
            m[n + j] = (int64_t)bk.in_len;
            m[2 * n + j] = (int64_t)(bk.out_off - o0);
            m[3 * n + j] = (int64_t)bk.out_len;
        }
        int32_t *const h_status = reinterpret_cast<int32_t *>(m + 4 * n);
        {
            std::atomic<int> bad{0};
            const size_t piece = (size_t)1 << 20;
            uint8_t *const hc = h_comp_.as<uint8_t>();
            parallel_for((int64_t)((comp_bytes + piece - 1) / piece), threads, [&](int64_t t) {
                const size_t a = (size_t)t * piece, e = std::min(comp_bytes, a + piece);
                if (!f.read(in0 + a, hc + a, e - a)) bad++;
            });
            if (bad) return fail(NPORE_E_INVALID, "cannot read the BGZF blocks of a window");
        }
        if (n) {
            const int64_t *const dm = d_meta_.as<int64_t>();
            HIP_TRY(hipMemcpyAsync(d_comp_.p, h_comp_.p, comp_bytes, hipMemcpyHostToDevice, s_));
            HIP_TRY(hipMemcpyAsync(d_meta_.p, h_meta_.p, n * 32, hipMemcpyHostToDevice, s_));
            HIP_TRY(hipEventRecord(e0_, s_));
            launch_inflate_blocks(d_comp_.as<uint8_t>(), dm, dm + n, d_out_.as<uint8_t>(), dm + 2 * n, dm + 3 * n, (int64_t)n,
                                  reinterpret_cast<int32_t *>(d_meta_.as<int64_t>() + 4 * n), s_);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(e1_, s_));
            HIP_TRY(hipMemcpyAsync(h_status, d_meta_.as<int64_t>() + 4 * n, n * 4, hipMemcpyDeviceToHost, s_));
            HIP_TRY(hipMemcpyAsync(dst, d_out_.p, out_bytes, hipMemcpyDeviceToHost, s_));
            HIP_TRY(hipStreamSynchronize(s_));
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, e0_, e1_));
            n_[INFL_LAUNCHES]++;
            n_[INFL_KERNEL_NS] += (int64_t)((double)ms * 1e6);
            n_[INFL_BYTES_UP] += (int64_t)comp_bytes;
            n_[INFL_BYTES_DOWN] += (int64_t)out_bytes;
        }
        // the CRCs, and the host decoder for what the device left
        std::atomic<int> bad{0};
        std::atomic<int64_t> on_device{0}, declined{0}, crc_failed{0};
        const bool crc = bgzf_check_crc();
        const uint8_t *const hc = h_comp_.as<uint8_t>();
        const int64_t per = 8;
        parallel_for(((int64_t)n + per - 1) / per, threads, [&](int64_t t) {
            for (size_t j = (size_t)(t * per); j < std::min(n, (size_t)((t + 1) * per)); j++) {
                const FastInflate::Job job{hc + m[j], (size_t)m[n + j], dst + m[2 * n + j], (size_t)m[3 * n + j]};
                bool ok = h_status[j] == 1;
                if (ok && crc && crc32_fast(0u, job.out, job.out_len) != rd32(job.in + job.in_len)) { ok = false; crc_failed++; }
                else if (!ok) declined++;
                if (ok) on_device++;
                else bad += inflate_blocks(&job, 1, 0, crc);
            }
        });
        n_[INFL_DEVICE] += on_device;
        n_[INFL_DECLINED] += declined;
        n_[INFL_CRC_FAILED] += crc_failed;
        return bad ? fail(NPORE_E_INVALID, "corrupt BGZF block") : NPORE_OK;
    }

private:
    int device_;
    hipStream_t s_ = nullptr;
    hipEvent_t e0_ = nullptr, e1_ = nullptr;
    HostBuf h_comp_, h_meta_;
    DevBuf d_comp_, d_meta_, d_out_;
    std::vector<size_t> which_;
    std::atomic<int64_t> n_[INFL_N] = {};
};

}  // namespace npore
