// staging.hpp -- host-pointer arguments of one call: the runtime's staging slots by name, and the call scope that stages through
// them.  Included by internal.hpp (after Runtime); not a header of its own.
#pragma once

namespace mi355
{

// One call of a compute entry point: runtime, stage lock, stream, and the device views of its pointer arguments (DESIGN.md 1,
// "Staging").  A device pointer is its own view.  A host array is copied into a staging slot -- or into a workspace of the handle
// the call runs on -- and, when it is an output, copied back by finish(), which then synchronises the stream once.  The status is
// sticky: after a failure every view is nullptr and finish() returns the first error, so a site chains its views and tests once.
// The destructor does no GPU work: a call that returns early copies nothing back.
//
// In device-pointer mode (aoclsparse_mi355_pointer_device, or inside a DeviceScope) a Conditional scope issues no HIP call and
// takes no lock: Runtime::is_device_pointer answers without asking the HIP runtime there, so every view is the pointer itself.
struct CallScope
{
    enum LockPolicy
    {
        Conditional, // the stage lock unless the pointer mode says that nothing will be staged
        Always // calls that also share a handle's workspaces, or use scratch slots whatever the pointers are
    };
    Runtime          &rt;
    hipStream_t       s  = nullptr;
    aoclsparse_status st = aoclsparse_status_success;

    explicit CallScope(LockPolicy policy)
        : rt(Runtime::get())
        , sl_(rt.stage_lock, std::defer_lock)
    {
        st = rt.init();
        if(st != aoclsparse_status_success)
            return;
        if(policy == Always || rt.pointer_mode != aoclsparse_mi355_pointer_device)
            sl_.lock();
        s = rt.stream();
    }
    CallScope(const CallScope &)            = delete;
    CallScope &operator=(const CallScope &) = delete;

    bool ok() const
    {
        return st == aoclsparse_status_success;
    }
    // a Conditional call that turns out to need scratch slots takes the lock late (before any handle's guard, as everywhere)
    void lock()
    {
        if(!sl_.owns_lock())
            sl_.lock();
    }

    // Device views of `p` (bytes long).  `where` is a StageSlot or a DeviceBuffer of the handle; at least one byte is allocated.
    // in: read only, copied in when `copy`;  inout: also copied back by finish() (unless the site says it copies back itself, or
    // that this call does not write the array);  out: copied back only.
    template <typename T, typename Where>
    const T *in(Where &&where, const T *p, size_t bytes, bool copy = true)
    {
        return static_cast<const T *>(view(where, p, bytes, ok() && rt.is_device_pointer(p), copy, false));
    }
    template <typename T, typename Where>
    T *inout(Where &&where, T *p, size_t bytes, bool copy_in, bool copy_back = true)
    {
        return static_cast<T *>(view(where, p, bytes, ok() && rt.is_device_pointer(p), copy_in, copy_back));
    }
    template <typename T, typename Where>
    T *out(Where &&where, T *p, size_t bytes)
    {
        return inout(where, p, bytes, false);
    }
    // the same for a site that has asked is_device_pointer(p) itself (each argument is asked about once per call)
    template <typename Where>
    void *view(Where &&where, const void *p, size_t bytes, bool is_dev, bool copy_in, bool copy_back)
    {
        return strided(where, p, 1, bytes, bytes, is_dev, copy_in, copy_back);
    }
    void *scratch(StageSlot slot, size_t bytes)
    {
        return ok() ? alloc(slot, bytes) : nullptr;
    }

    // Strided dense operands: `outer` lines of `inner` elements, `ld` apart; the extent is (outer - 1) * ld + inner elements (the
    // last line carries no ld padding: BLAS convention, and a column shard of a row-major matrix starts some elements into its first
    // row).  ONLY the `inner` elements of each line move; the ld padding -- which for a column shard of a row-major matrix is the
    // other shards' columns -- is neither sent nor, on the way back, written (round 3: the contiguous-span copy of round 2 rewrote
    // it with the values it had read, which is a lost update as soon as another thread -- another device's worker of ?csrmm_multi --
    // owns those columns, and sent 8 x the bytes a 1/8 shard needs).  One contiguous copy when ld == inner or outer == 1.
    template <typename T>
    const T *dense_in(StageSlot slot, const T *p, aoclsparse_int outer, aoclsparse_int inner, aoclsparse_int ld, bool copy = true)
    {
        return static_cast<const T *>(dense(slot, p, sizeof(T), outer, inner, ld, copy, false));
    }
    template <typename T>
    T *dense_inout(StageSlot slot, T *p, aoclsparse_int outer, aoclsparse_int inner, aoclsparse_int ld, bool copy_in)
    {
        return static_cast<T *>(dense(slot, p, sizeof(T), outer, inner, ld, copy_in, true));
    }

    // copies the registered outputs back in registration order, then synchronises the stream once if there were any
    aoclsparse_status finish()
    {
        if(!ok())
            return st;
        for(int i = 0; i < nback_; i++)
            if((st = copy(back_[i].host, back_[i].dev, back_[i], hipMemcpyDeviceToHost)) != aoclsparse_status_success)
                return st;
        if(nback_ && hipStreamSynchronize(s) != hipSuccess)
            st = aoclsparse_status_internal_error;
        nback_ = 0;
        return st;
    }

private:
    struct Span // `lines` lines of `width` bytes, `pitch` bytes apart
    {
        void  *host, *dev;
        size_t lines, width, pitch;
    };
    std::unique_lock<std::recursive_mutex> sl_;
    Span                                   back_[3];
    int                                    nback_ = 0;

    void *alloc(StageSlot slot, size_t bytes)
    {
        void *d = nullptr;
        st      = rt.staging(slot, bytes, &d);
        return ok() ? d : nullptr;
    }
    void *alloc(DeviceBuffer &buf, size_t bytes)
    {
        st = buf.alloc(bytes);
        return ok() ? buf.ptr : nullptr;
    }
    aoclsparse_status copy(void *dst, const void *src, const Span &sp, hipMemcpyKind kind)
    {
        if(!sp.lines || !sp.width)
            return aoclsparse_status_success;
        if(sp.lines == 1)
            MI355_HIP_TRY(hipMemcpyAsync(dst, src, sp.width, kind, s));
        else
            MI355_HIP_TRY(hipMemcpy2DAsync(dst, sp.pitch, src, sp.pitch, sp.width, sp.lines, kind, s));
        return aoclsparse_status_success;
    }
    template <typename Where>
    void *strided(Where &&where, const void *p, size_t lines, size_t width, size_t pitch, bool is_dev, bool copy_in, bool copy_back)
    {
        if(!ok())
            return nullptr;
        if(is_dev)
            return const_cast<void *>(p);
        const size_t bytes = lines ? (lines - 1) * pitch + width : 0;
        void        *d     = alloc(where, bytes ? bytes : 1);
        if(!d)
            return nullptr;
        const Span sp{const_cast<void *>(p), d, lines, width, pitch};
        if(copy_in)
            st = copy(d, p, sp, hipMemcpyHostToDevice);
        if(copy_back)
            back_[nback_++] = sp;
        return ok() ? d : nullptr;
    }
    void *dense(StageSlot slot, const void *p, size_t elem, aoclsparse_int outer, aoclsparse_int inner, aoclsparse_int ld, bool copy_in,
                bool copy_back)
    {
        const bool   is_dev = ok() && rt.is_device_pointer(p);
        const size_t lines  = outer > 0 && inner > 0 ? (size_t)outer : 0;
        if(ld == inner || lines <= 1) // one span
            return strided(slot, p, lines ? 1 : 0, lines ? elem * ((lines - 1) * (size_t)ld + (size_t)inner) : 0, 0, is_dev, copy_in,
                           copy_back);
        return strided(slot, p, lines, elem * (size_t)inner, elem * (size_t)ld, is_dev, copy_in, copy_back);
    }
};

} // namespace mi355
