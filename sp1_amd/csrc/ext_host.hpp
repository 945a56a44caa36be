// sp1_amd/csrc/ext_host.hpp — the host-side field helpers the sumcheck provers share (gkr.hip, jagged.hip): the extension
// field's operators, the partial-Lagrange (eq) table and multilinear evaluation on the host, and the arena buffer with typed
// views that the small uploads go into. Everything lives in sp1hip::ext_host and is pulled in with a using-directive: the
// only class named sp1hip::DeviceBuf stays basefold_host.hpp's.
#pragma once
#include <algorithm>
#include <vector>

#include "kb31.hpp"
#include "round_sync.hpp"
#include "tensor_table.hpp"

namespace sp1hip {
namespace ext_host {

using Ext = kb::Ext;

struct DeviceBuf : AsyncScratch {
    uint32_t* u32() const { return (uint32_t*)p; }
    Ext* ext() const { return (Ext*)p; }
};

inline Ext operator+(const Ext& a, const Ext& b) { return kb::ext_add(a, b); }
inline Ext operator-(const Ext& a, const Ext& b) { return kb::ext_sub(a, b); }
inline Ext operator*(const Ext& a, const Ext& b) { return kb::ext_mul(a, b); }
inline Ext ext_c(uint32_t canonical) { return kb::ext_from_base(kb::to_monty(canonical)); }
inline int log2_ceil(uint64_t x) { int l = 0; while (((uint64_t)1 << l) < x) l++; return l; }

inline std::vector<Ext> partial_lagrange_host(const std::vector<Ext>& pt) {
    std::vector<Ext> ev{kb::ext_one()};
    for (const Ext& x : pt) {
        std::vector<Ext> nx(ev.size() * 2);
        for (size_t i = 0; i < ev.size(); i++) { const Ext pr = ev[i] * x; nx[2 * i] = ev[i] - pr; nx[2 * i + 1] = pr; }
        ev.swap(nx);
    }
    return ev;
}
// vals may be shorter than 2^|pt| (the missing tail is zero)
inline Ext eval_mle_host(const std::vector<Ext>& vals, const std::vector<Ext>& pt) {
    const std::vector<Ext> eq = partial_lagrange_host(pt);
    Ext acc = kb::ext_zero();
    for (size_t i = 0; i < vals.size() && i < eq.size(); i++) acc = acc + eq[i] * vals[i];
    return acc;
}

inline int upload(DeviceBuf& buf, const void* src, size_t bytes, hipStream_t s, PinnedStage& stage) {
    SP1HIP_TRY(buf.alloc(std::max<size_t>(bytes, 16), s));
    return stage.upload(buf.p, src, bytes);
}

}  // namespace ext_host
}  // namespace sp1hip
