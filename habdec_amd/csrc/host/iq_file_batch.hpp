// Batched IQ file ingest: S independent IQ files read in lock step into one push slab [S][stride].
//
// One file behaves like the reference's IQSource_File<float>::get (code/IQSource/IQSource_File.h:124-172): raw
// interleaved float32 I,Q, little-endian, no header (:156-157); a read returns what is left; the end of file is only
// NOTICED by the read that runs into it (std::ifstream's eofbit), and the call AFTER that one rewinds when looping
// (:141-155) -- so a file whose length is a whole number of requests delivers one empty read before it starts over,
// exactly like the reference.  The realtime throttle (:165-169) is optional.
//
// The batch adds what a batched decoder needs: every stream hands over a whole multiple of `granule` samples per round
// (the total decimation factor: Decoder::process consumes floor(n/D)*D samples and keeps the rest queued,
// Decoder.h:429-435); the remainder is carried in front of the stream's next round.
//
// Packed files (HD_IQ_CS16 / CS8 / CU8, host/iq_convert.hpp): the same reader with bytes-per-sample 4 or 2 instead of 8 -- count, reads, the carry and
// rewinds are counted in samples and hold the file's own bytes; next_raw hands them on as they are, next converts them to floats.
#pragma once
#include <stdint.h>

#include <chrono>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "iq_convert.hpp"

namespace hd {

class IqFile {
  public:
    bool open(const std::string& path, bool loop, uint32_t bps = 8u)
    {
        path_ = path; loop_ = loop; bps_ = bps;
        {   // IQSource_File::init: count_ = filesize / sizeof(complex<float>)
            std::ifstream in(path, std::ifstream::ate | std::ifstream::binary);
            if (!in.is_open()) return false;
            count_ = (uint64_t)in.tellg() / bps_;
        }
        f_.open(path, std::ios::binary);
        return f_.is_open();
    }
    uint64_t count() const { return count_; }
    bool loops() const { return loop_; }
    uint64_t rewinds() const { return rewinds_; }
    // IQSource_File::get: up to `want` complex samples into dst (bps bytes each: 2 floats in a cf32 file); returns the number read
    size_t get(void* dst, size_t want)
    {
        if (!f_.is_open()) return 0;
        if (f_.eof()) {
            if (!loop_) return 0;
            f_.clear();
            f_.seekg(0);
            ++rewinds_;
        }
        const uint64_t n = want < count_ ? want : count_;
        f_.read(static_cast<char*>(dst), (std::streamsize)(n * bps_));
        return (size_t)f_.gcount() / bps_;
    }

  private:
    std::ifstream f_;
    std::string path_;
    bool loop_ = false;
    uint64_t count_ = 0, rewinds_ = 0;
    uint32_t bps_ = 8;
};

class IqFileBatch {
  public:
    // chunk: samples requested per stream and round (the reference asks for 65536, websocketServer/main.cpp:235)
    bool open(const std::vector<std::string>& paths, bool loop, uint32_t chunk, uint32_t granule, double realtime_rate = 0.0, int fmt = HD_IQ_CF32)
    {
        if (paths.empty() || !chunk || !granule || chunk < granule || !iq_bytes(fmt)) return false;
        chunk_ = chunk; granule_ = granule; rate_ = realtime_rate; fmt_ = fmt; bps_ = (uint32_t)iq_bytes(fmt); raw_.clear();
        files_.clear(); carry_.clear(); carry_n_.assign(paths.size(), 0);
        for (const auto& p : paths) {
            files_.emplace_back(new IqFile);
            if (!files_.back()->open(p, loop, bps_)) { files_.clear(); return false; }
            carry_.emplace_back((size_t)granule * bps_, (unsigned char)0);
        }
        return true;
    }
    // Rounds smaller than `n` samples (but not empty) are held back and joined with the stream's next round: the engine rejects
    // chunks shorter than its stage histories (undefined behaviour in the reference, Q4), and a file's tail may be that short.
    void set_min_take(uint32_t n)
    {
        min_take_ = n;
        for (auto& c : carry_) if (c.size() < ((size_t)n + granule_) * bps_) c.resize(((size_t)n + granule_) * bps_, (unsigned char)0);
    }
    bool looping() const { for (const auto& f : files_) if (f->loops()) return true; return false; }
    uint32_t streams() const { return (uint32_t)files_.size(); }
    uint32_t chunk() const { return chunk_; }
    int fmt() const { return fmt_; }
    uint32_t bytes_per_sample() const { return bps_; }
    const IqFile& file(uint32_t s) const { return *files_[s]; }
    // Fill slab[s*stride*2 ...] (stride in complex samples, >= chunk) and n_out[s] (a multiple of granule, <= chunk).
    // Returns the number of streams that read anything this round (0 = every file is exhausted and not looping).
    // A packed batch: the round's bytes through iq_convert, n_out[s] samples per stream.
    uint32_t next(float* slab, size_t stride, uint32_t* n_out)
    {
        if (fmt_ == HD_IQ_CF32) return next_raw(slab, stride, n_out);
        if (raw_.size() < files_.size() * (size_t)chunk_ * bps_) raw_.resize(files_.size() * (size_t)chunk_ * bps_);
        const uint32_t alive = next_raw(raw_.data(), chunk_, n_out);
        for (size_t s = 0; s < files_.size(); ++s) iq_convert(fmt_, raw_.data() + s * chunk_ * bps_, n_out[s], slab + s * stride * 2);
        return alive;
    }
    // The same round in the files' own bytes: stream s at byte s * stride * bytes_per_sample() of the slab.
    uint32_t next_raw(void* slab_bytes, size_t stride, uint32_t* n_out)
    {
        unsigned char* slab = static_cast<unsigned char*>(slab_bytes);
        const size_t B = bps_;
        uint32_t alive = 0;
        uint64_t most = 0;
        for (size_t s = 0; s < files_.size(); ++s) {
            unsigned char* dst = slab + s * stride * B;
            const uint32_t c = carry_n_[s];
            if (c) std::memcpy(dst, carry_[s].data(), (size_t)c * B);
            const size_t got = files_[s]->get(dst + (size_t)c * B, chunk_ - c);
            if (got) ++alive;
            most = got > most ? got : most;
            const uint32_t total = c + (uint32_t)got;
            uint32_t rem = total % granule_;
            if (total - rem && total - rem < min_take_ && total < chunk_) rem = total;     // too short for the engine: wait for more
            n_out[s] = total - rem;
            if (rem) std::memcpy(carry_[s].data(), dst + (size_t)(total - rem) * B, (size_t)rem * B);
            carry_n_[s] = rem;
        }
        if (rate_ > 0.0 && most)   // IQSource_File.h:165-169, once per round for the batch
            std::this_thread::sleep_for(std::chrono::duration<double, std::milli>((double)(size_t)((double)most / rate_ * 1000)));
        return alive;
    }

  private:
    std::vector<std::unique_ptr<IqFile>> files_;
    std::vector<std::vector<unsigned char>> carry_;
    std::vector<unsigned char> raw_;       // next() of a packed batch: the round before conversion, [S][chunk]
    std::vector<uint32_t> carry_n_;
    uint32_t chunk_ = 0, granule_ = 1, min_take_ = 0, bps_ = 8;
    int fmt_ = HD_IQ_CF32;
    double rate_ = 0.0;
};

}  // namespace hd

// handle of the C ABI (habdec_amd_host.h): shared by host_api.cpp (reader) and engine.cpp (the pump that feeds an engine)
struct hd_host_iqfiles { hd::IqFileBatch batch; };
