// Where a streaming feed's ops are -- part of api.hip's translation unit, in front of stream.inc and eval_stream.inc.
//
// rv_stream_feed / rv_eval_stream_feed read a host array; rv_stream_feed_device / rv_eval_stream_feed_device take one in device
// memory.  The feed pipelines (stream_feed_impl, eval_stream_feed_impl) are the same for both: they ask a FeedOps for what they need
// to know of a piece -- its digest, its mask and event counts, whether it is all GF(2) -- and a PieceOnHost for its ops when the
// host compiler has to read them.
//   host feed:    the three loops over the caller's array (ops_digest, count_masks / count_events, piece_all_gf2), as ever; the
//                 ops are where they are.
//   device feed:  one kernel sums all of it for every piece of the feed up front (piece_sums.hip; one small copy back), the device
//                 compiler reads d_ops + offset in place, and only a piece the HOST compiler must see is copied down: into a
//                 page-locked slot of the context (rv_ctx::OpsSlots), by the thread that compiles it, for the length of the compile.

static uint64_t ops_digest(const rv_op* ops, size_t n, uint64_t first_index);  // (stream.inc)

struct FeedOps {
    rv_ctx* ctx = nullptr;
    const rv_op* host = nullptr;  // the caller's array (host feed)
    const rv_op* dev = nullptr;   // ... or its device array
    bool device = false;
    const std::vector<size_t>* cut = nullptr;  // piece i = ops [cut[i], cut[i + 1])
    std::vector<PieceSums> sums;               // device feed: per piece (load_sums)
    size_t slot_bytes = 0;                     // device feed: bytes of the longest piece

    FeedOps(rv_ctx* ctx_, const rv_op* ops, bool device_, const std::vector<size_t>& cut_)
        : ctx(ctx_), host(device_ ? nullptr : ops), dev(device_ ? ops : nullptr), device(device_), cut(&cut_) {}
    size_t n_pieces() const { return cut->size() - 1; }
    size_t at(size_t i) const { return (*cut)[i]; }
    size_t len(size_t i) const { return (*cut)[i + 1] - (*cut)[i]; }

    // first_op: the stream position of the feed's first op
    uint64_t digest(size_t i, uint64_t first_op) const { return device ? sums[i].digest : ops_digest(host + at(i), len(i), first_op + at(i)); }
    void counts(size_t i, uint64_t* m2, uint64_t* m64, StreamEvents* ev) const {
        if (!device) {
            count_masks(host + at(i), len(i), m2, m64);
            count_events(host + at(i), len(i), ev);
            return;
        }
        const PieceSums& s = sums[i];
        *m2 = s.masks2, *m64 = s.masks64;
        ev->in2 = s.in2, ev->rec2 = s.rec2, ev->pre2 = s.pre2, ev->on64 = s.on64, ev->pre64 = s.pre64;
    }
    bool all_gf2(size_t i) const { return device ? sums[i].not_gf2 == 0 : piece_all_gf2(host + at(i), len(i)); }
    bool no_b2a(size_t i) const { return device ? sums[i].not_z64 == 0 : piece_no_b2a(host + at(i), len(i)); }
    // the pieces a stream with these compile flags sends to the device compiler: all-GF(2) ones; under RV_COMPILE_DEVICE_Z64 every
    // piece without a B2A op; with RV_COMPILE_DEVICE_B2A every piece (an error in one comes back through the fallback)
    bool for_device(size_t i, uint32_t compile_flags) const {
        if (!(compile_flags & RV_COMPILE_DEVICE)) return false;
        if ((compile_flags & RV_COMPILE_DEVICE_Z64) && (compile_flags & RV_COMPILE_DEVICE_B2A)) return true;
        return (compile_flags & RV_COMPILE_DEVICE_Z64) ? no_b2a(i) : all_gf2(i);
    }
    // piece i through the chunk mode of the device compiler: a host feed's ops go up (counted as op traffic), a device feed's are
    // read where they are
    int compile_on_device(size_t i, size_t z64_wires, size_t gf2_wires, const ChunkStart& cs, Compiled& cc, DevCompileKeep* keep, double laps[3] = nullptr,
                          uint32_t compile_flags = 0) const {
        return compile_chunk_on_device(ctx, device ? nullptr : host + at(i), device ? dev + at(i) : nullptr, len(i), z64_wires, gf2_wires, cs, cc, keep, laps,
                                       &g_op_bytes_h2d, compile_flags);
    }

    // Device feed: the sums of every piece (on the context's stream, one wait), the copy stream, and how many slots PieceOnHost may
    // hold at once: one per thread that compiles, within 512 MiB of page-locked memory, two at least.  Main thread, before the workers.
    int load_sums(uint64_t first_op, unsigned n_threads) {
        if (!device) return RV_OK;
        const size_t np = n_pieces();
        sums.assign(np, PieceSums{});
        if (!np) return RV_OK;
        size_t longest = 0;
        for (size_t i = 0; i < np; i++) longest = std::max(longest, len(i));
        slot_bytes = std::max<size_t>(longest, 1) * sizeof(rv_op);
        {
            std::lock_guard<std::mutex> lk(ctx->ops_slots.mu);
            ctx->ops_slots.max_slots = std::max<size_t>(2, std::min<size_t>({(size_t)n_threads + 1, ((size_t)512 << 20) / slot_bytes, rv_ctx::OpsSlots::MAX}));
        }
        if (!ctx->stream_ops) HIPCHK(hipStreamCreateWithFlags(&ctx->stream_ops, hipStreamNonBlocking));
        uint64_t* d_cut = nullptr;
        PieceSums* d_sums = nullptr;
        int rc;
        if ((rc = dalloc(ctx, np + 1, &d_cut)) || (rc = dalloc(ctx, np, &d_sums))) {
            ctx->release(d_cut);
            return rc;
        }
        const std::vector<uint64_t> c64(cut->begin(), cut->end());
        hipStream_t st = ctx->stream;
        hipError_t e = hipMemcpyAsync(d_cut, c64.data(), c64.size() * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            launch_piece_sums(st, dev, d_cut, np, longest, first_op, d_sums);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(sums.data(), d_sums, np * sizeof(PieceSums), hipMemcpyDeviceToHost, st);
        const hipError_t es = hipStreamSynchronize(st);  // (also after a failure: c64 and sums leave scope)
        ctx->release(d_cut);
        ctx->release(d_sums);
        if (e == hipSuccess) e = es;
        return e == hipSuccess ? RV_OK : hip_fail(e, "piece sums of a device feed", __FILE__, __LINE__);
    }
};

// A piece's ops where the host compiler can read them, for as long as this object lives.  A host feed: the caller's array.  A device
// feed: a page-locked slot of the context, filled here (any thread) -- waits while every slot is held by another compile.
class PieceOnHost {
  public:
    PieceOnHost(const FeedOps& f, size_t i) {
        if (!f.device) {
            ops_ = f.host + f.at(i);
            return;
        }
        ctx_ = f.ctx;
        const size_t bytes = f.len(i) * sizeof(rv_op);
        if (hipSetDevice(ctx_->device) != hipSuccess) {
            rc_ = hip_fail(hipGetLastError(), "hipSetDevice", __FILE__, __LINE__);
            return;
        }
        uint8_t* h = nullptr;
        if ((rc_ = take(std::max(bytes, f.slot_bytes), &h))) return;
        hipError_t e = hipMemcpyAsync(h, f.dev + f.at(i), bytes, hipMemcpyDeviceToHost, ctx_->stream_ops);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx_->stream_ops);
        if (e != hipSuccess) {
            rc_ = hip_fail(e, "copy of a device feed's piece to the host", __FILE__, __LINE__);
            return;
        }
        g_op_bytes_d2h.fetch_add(bytes, std::memory_order_relaxed);
        ops_ = (const rv_op*)h;
    }
    ~PieceOnHost() {
        if (slot_ < 0) return;
        {
            std::lock_guard<std::mutex> lk(ctx_->ops_slots.mu);
            ctx_->ops_slots.slot[(size_t)slot_].busy = false;
        }
        ctx_->ops_slots.cv.notify_all();
    }
    PieceOnHost(const PieceOnHost&) = delete;
    PieceOnHost& operator=(const PieceOnHost&) = delete;
    int rc() const { return rc_; }
    const rv_op* ops() const { return ops_; }

  private:
    // A free slot with a buffer of at least `bytes`, claimed (busy) under the lock: one that is large enough, else the first free one
    // of the max_slots in use, whose buffer is then replaced; else wait for a compile to give one back.  The page-locking calls run
    // outside the lock -- the claimed slot's p and cap are this thread's until it clears busy -- so other threads' hand-backs do not
    // wait behind them.  *buf: the buffer.  RV_E_NOMEM when page-locked memory is refused and no other compile holds a slot.
    int take(size_t bytes, uint8_t** buf) {
        rv_ctx::OpsSlots& S = ctx_->ops_slots;
        std::unique_lock<std::mutex> lk(S.mu);
        for (;;) {
            int pick = -1;
            bool any_busy = false;
            const size_t n = std::min(S.max_slots, rv_ctx::OpsSlots::MAX);
            for (size_t k = 0; k < n; k++) {
                if (S.slot[k].busy)
                    any_busy = true;
                else if (S.slot[k].cap >= bytes && (pick < 0 || S.slot[(size_t)pick].cap < bytes))
                    pick = (int)k;
                else if (pick < 0)
                    pick = (int)k;
            }
            if (pick < 0) {
                S.cv.wait(lk);
                continue;
            }
            rv_ctx::OpsSlots::Slot& sl = S.slot[(size_t)pick];
            sl.busy = true;
            if (sl.cap >= bytes) {
                slot_ = pick;
                *buf = sl.p;
                return RV_OK;
            }
            uint8_t* old = sl.p;
            sl.p = nullptr, sl.cap = 0;
            lk.unlock();
            if (old) (void)hipHostFree(old);
            uint8_t* p = nullptr;
            const bool ok = hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) == hipSuccess;
            if (!ok) (void)hipGetLastError(), p = nullptr;
            lk.lock();
            if (ok) {
                sl.p = p, sl.cap = bytes;
                slot_ = pick;
                *buf = p;
                return RV_OK;
            }
            sl.busy = false;
            if (!any_busy) {
                g_last_error = "device feed: no page-locked memory for a piece's ops";
                return RV_E_NOMEM;
            }
            S.cv.wait(lk);  // (a compile that holds a slot will give it back)
        }
    }
    rv_ctx* ctx_ = nullptr;
    int slot_ = -1;
    int rc_ = RV_OK;
    const rv_op* ops_ = nullptr;
};

// Test hook: the eight sums of every piece of a feed -- ops [0, n_ops) at stream position first_index, cut every piece_ops ops (0: one
// piece, also when it is empty) -- as a host feed makes them (the three loops) and as a device feed does (the ops go up, one launch
// of the kernel over the cut table): per piece digest, GF(2) and Z64 masks, in2, rec2, pre2, on64, pre64.  host_out / dev_out:
// [pieces][8], pieces = max(1, ceil(n_ops / piece_ops)).
extern "C" int rv_hook_stream_piece_sums(rv_ctx* ctx, const rv_op* ops, size_t n_ops, uint64_t first_index, size_t piece_ops, uint64_t* host_out,
                                         uint64_t* dev_out) {
    return guarded([&]() -> int {
        if (!ctx || !host_out || !dev_out || (n_ops && !ops)) return RV_E_ARG;
        HIPCHK(hipSetDevice(ctx->device));
        std::vector<size_t> cut = {0};
        for (size_t at = 0; piece_ops && at + piece_ops < n_ops; at += piece_ops) cut.push_back(at + piece_ops);
        cut.push_back(n_ops);
        rv_op* d_ops = nullptr;
        if (int rc = upload_ops(ctx, ops, n_ops, &d_ops)) return rc;
        FeedOps on_host(ctx, ops, false, cut), on_dev(ctx, d_ops, true, cut);
        const int rc = on_dev.load_sums(first_index, 1);  // (waits for the stream: the upload too)
        ctx->release(d_ops);
        if (rc) return rc;
        const FeedOps* both[2] = {&on_host, &on_dev};
        uint64_t* out[2] = {host_out, dev_out};
        for (int k = 0; k < 2; k++)
            for (size_t i = 0; i + 1 < cut.size(); i++) {
                uint64_t* o = out[k] + 8 * i;
                StreamEvents ev;
                o[0] = both[k]->digest(i, first_index);
                both[k]->counts(i, &o[1], &o[2], &ev);
                o[3] = ev.in2, o[4] = ev.rec2, o[5] = ev.pre2, o[6] = ev.on64, o[7] = ev.pre64;
            }
        return RV_OK;
    });
}
