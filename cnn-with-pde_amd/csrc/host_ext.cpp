// Native host path of the launch-bound layer calls: the autograd node of one implicit diffusion layer
// (functional.adi_diffuse: mnist_test.py:44-198, fashion_mnist.py:18-196, the C = 1 shapes the reference trains on) written
// against torch's C++ autograd and the C ABI of include/pdecnn.h.  Same calls, same arguments and the same order of
// launches as functional._AdiFn (which stays the general path: coefficient-maxima sinks, lagged plans), and likewise for
// the layers with a channel operator (SmallFn, MixedFn, MultiFn against functional._AdiSmallFn, _AdiMixedFn, _AdiMultiFn:
// the helpers ahead of the nodes mirror functional.py's, decision by decision); what goes is the
// interpreter between them — at (64,1,28,28) the kernels of a forward + backward take 0.1 ms on the device and the Python
// around them 0.17 ms on the host.
//
// Nothing here computes: tensors are allocated through torch's caching allocator, every result comes from the HIP kernels
// of libpdecnn_hip.so on torch's current stream.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <hip/hip_runtime_api.h>
#include <torch/csrc/autograd/functions/basic_ops.h>

#include <atomic>
#include <chrono>
#include <map>
#include <tuple>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/pdecnn.h"

namespace {

using torch::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

const char* err_text(int rc) {
    switch (rc) {
        case -1: return "PDE_E_BADARG (null or misaligned pointer, bad dimension or enum)";
        case -2:
            return "PDE_E_UNSUPPORTED_N (line length outside [2, 128], or a per-step / one-launch entry point at a line length "
                   "without fused kernels: those exist for multiples of 4 in [8, 32])";
        case -3: return "PDE_E_TOO_MANY_SWEEPS";
        case -4: return "PDE_E_LAUNCH (HIP launch failed)";
        case -5: return "PDE_E_WORKSPACE (workspace too small or misaligned)";
    }
    return "unknown error";
}

// A failed call of the C ABI: reaches Python as _lib.PdeError (a RuntimeError), like the ctypes path's
struct PdeFailure : public std::runtime_error {
    using std::runtime_error::runtime_error;
};
PyObject* g_error_class = nullptr;

#define PDE_REQUIRE(cond, ...)                                  \
    do {                                                        \
        if (!(cond)) throw PdeFailure(c10::str(__VA_ARGS__));   \
    } while (0)

void check(int rc, const char* what) {
    if (rc != 0) throw PdeFailure(std::string(what) + " failed: " + err_text(rc));
}

// ---- the way the per-sweep coefficient maxima reach the host: pinned slots, one event each -------------------------------
// pde_adi_forward writes the maxima into the slot and records the event right behind its factorisation kernel; the
// backward plans its checkpoints from them (functional.plan_checkpoints).  A slot is held from a forward until its node
// dies (a tensor over the slot's memory, kept in the node, hands it back from its deleter).
struct Slot {
    float* host = nullptr;
    hipEvent_t ev = nullptr;
    std::atomic<bool> busy{false};
    bool pooled = true;
};

constexpr int kRing = 256;
constexpr int kSlotFloats = PDE_MAX_SWEEPS * 4;

struct Ring {
    std::mutex mu;
    std::vector<std::unique_ptr<Slot>> slots;
    float* pool = nullptr;
    int next = 0;
};

Ring* ring_of(int dev) {
    // (never destroyed: a slot's ticket may be released — its deleter run — while the process is exiting, after static
    //  destructors of this library would have run)
    static std::mutex& mu = *new std::mutex();
    static std::vector<std::unique_ptr<Ring>>& rings = *new std::vector<std::unique_ptr<Ring>>();
    std::lock_guard<std::mutex> g(mu);
    if ((int)rings.size() <= dev) rings.resize(dev + 1);
    if (!rings[dev]) {
        auto r = std::make_unique<Ring>();
        TORCH_CHECK(hipHostMalloc((void**)&r->pool, sizeof(float) * kSlotFloats * kRing, hipHostMallocDefault) == hipSuccess,
                    "hipHostMalloc of the coefficient-maxima ring failed");
        for (int i = 0; i < kRing; ++i) {
            auto s = std::make_unique<Slot>();
            s->host = r->pool + (size_t)i * kSlotFloats;
            TORCH_CHECK(hipEventCreateWithFlags(&s->ev, hipEventDisableTiming) == hipSuccess, "hipEventCreate failed");
            r->slots.push_back(std::move(s));
        }
        rings[dev] = std::move(r);
    }
    return rings[dev].get();
}

Slot* acquire_slot(int dev) {
    Ring* r = ring_of(dev);
    {
        std::lock_guard<std::mutex> g(r->mu);
        for (int off = 0; off < kRing; ++off) {
            int i = (r->next + off) % kRing;
            Slot* s = r->slots[i].get();
            if (!s->busy.load(std::memory_order_acquire)) {
                s->busy.store(true, std::memory_order_release);
                r->next = (i + 1) % kRing;
                return s;
            }
        }
    }
    // every slot is held by a node whose backward is outstanding: a slot of its own, freed with the node
    Slot* s = new Slot();
    s->pooled = false;
    s->busy.store(true);
    TORCH_CHECK(hipHostMalloc((void**)&s->host, sizeof(float) * kSlotFloats, hipHostMallocDefault) == hipSuccess,
                "hipHostMalloc failed");
    TORCH_CHECK(hipEventCreateWithFlags(&s->ev, hipEventDisableTiming) == hipSuccess, "hipEventCreate failed");
    return s;
}

void release_slot(Slot* s) {
    if (s->pooled) {
        s->busy.store(false, std::memory_order_release);
        return;
    }
    (void)hipEventDestroy(s->ev);
    (void)hipHostFree(s->host);
    delete s;
}

// A CPU tensor over the slot's pinned floats whose deleter returns the slot: stored in the node, it ties the slot's
// life to the node's without a class registration.
Tensor slot_ticket(Slot* s, int n) {
    return at::from_blob(s->host, {n}, [s](void*) { release_slot(s); }, at::TensorOptions().dtype(at::kFloat));
}

void wait_event(hipEvent_t ev) {
    // Expected within microseconds of the device reaching the factorisation kernel — but the device may still be busy with
    // the previous step's backward when the host gets here (a device-bound loop: the host runs one pass ahead), so the poll
    // is bounded by TIME, not by a number of queries: a query of a pending event costs 15 ns on some hosts and 1 us on
    // others, and a blocking hipEventSynchronize costs 100-150 us to wake up from (0.60 ms per headline step instead of
    // 0.49 where 20,000 queries ran out first).
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        for (int i = 0; i < 256; ++i)
            if (hipEventQuery(ev) == hipSuccess) return;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
    }
    TORCH_CHECK(hipEventSynchronize(ev) == hipSuccess, "hipEventSynchronize failed");
}

// functional.plan_checkpoints: bit s set = keep the state after sweep s instead of rebuilding it
void plan_checkpoints(const float* kmax, int n, double amax, uint64_t mask[2]) {
    mask[0] = mask[1] = 0;
    double amp = 1.0;
    for (int s = n - 1; s >= 1; --s) {
        amp *= 1.0 + 4.0 * (double)kmax[s];
        if (amp > amax) {
            int b = s - 1;
            mask[b >> 6] |= 1ull << (b & 63);
            amp = 1.0;
        }
    }
}

int popcount2(const uint64_t m[2]) { return __builtin_popcountll(m[0]) + __builtin_popcountll(m[1]); }

// functional._aligned: the tensor as the library may be handed it (pdecnn.h, "Alignment": tensors, coefficient planes and
// matrices begin on 16 bytes) — itself when it does, as every fresh allocation, else a contiguous copy of its own.
// contiguous() leaves a contiguous view where its storage offset puts it: u[1:], a parameter cut from one flat buffer.
// Running statistics are updated in place one element at a time and are passed as they are.
Tensor aligned(Tensor t) {
    if (!t.defined() || (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0) return t;
    return t.clone(at::MemoryFormat::Contiguous);
}

// functional._as_chw: (C,N,N) fp32 contiguous view of a coefficient tensor given as (N,N), (1,N,N) or (C,N,N)
Tensor as_chw(const Tensor& p, int64_t C, int64_t N) {
    Tensor q = p.detach();
    if (q.dim() == 2) q = q.unsqueeze(0);
    PDE_REQUIRE(q.dim() == 3 && q.size(0) == C && q.size(1) == N && q.size(2) == N, "coefficient of shape ", p.sizes(),
                " does not match (", C, ",", N, ",", N, ")");
    if (q.scalar_type() != at::kFloat) q = q.to(at::kFloat);
    return aligned(q.contiguous());
}

// tensor types the kernels take as they are (functional._IO_TYPES; the caller widens an fp16 input off the float16 route)
bool io_type(const Tensor& u) {
    return u.scalar_type() == at::kFloat || u.scalar_type() == at::kBFloat16 || u.scalar_type() == at::kHalf;
}
int32_t io_of(const Tensor& u) {
    return u.scalar_type() == at::kBFloat16 ? PDE_IO_BF16 : (u.scalar_type() == at::kHalf ? PDE_IO_F16 : PDE_IO_F32);
}

Tensor bytes(size_t n, const Tensor& like) {
    return at::empty({(int64_t)std::max<size_t>(n, 256)}, like.options().dtype(at::kByte));
}

// _lib.bwd_input_enabled: PDE_BWD_INPUT=0 keeps the full backward for calls whose coefficients take no gradient
bool bwd_input_enabled() {
    static const bool on = [] { const char* e = std::getenv("PDE_BWD_INPUT"); return !(e && e[0] == '0' && e[1] == 0); }();
    return on;
}

// what a call keeps for its backward: nothing, everything the full backward reads, or — coefficients frozen, gradient
// for the input alone — the coefficient views and the factorisation only (pde_adi_backward_input reads neither y nor u)
constexpr int64_t kGradNone = 0, kGradFull = 1, kGradInput = 2;
int64_t grad_mode_of(const Tensor& u, bool params) {
    if (!at::GradMode::is_enabled()) return kGradNone;
    if (params) return kGradFull;
    if (!u.requires_grad()) return kGradNone;
    return bwd_input_enabled() ? kGradInput : kGradFull;
}
int64_t adi_grad_mode(const Tensor& u, const Tensor& ab, const Tensor& bb, const Tensor& asl, const Tensor& bsl) {
    return grad_mode_of(u, ab.requires_grad() || bb.requires_grad() || asl.requires_grad() || bsl.requires_grad());
}

// ---- what the four nodes below share: each decision is taken in one place (functional.py cuts its nodes the same way;
// tests/test_gpu_node_calls.py holds the two mirrors to the same bits) ---------------------------------------------------
void require_cuda(std::initializer_list<const Tensor*> ts) {
    for (const Tensor* t : ts)
        PDE_REQUIRE(!t->defined() || t->is_cuda(), "libpdecnn_hip operators need CUDA/HIP tensors (there is no CPU fallback)");
}

float* fptr(const Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }
void* vptr(const Tensor& t) { return t.defined() ? t.data_ptr() : nullptr; }
// the four coefficient views (or their gradients) as the C ABI takes them, one argument each
#define PDE_F4(p) (p)[0].data_ptr<float>(), (p)[1].data_ptr<float>(), (p)[2].data_ptr<float>(), (p)[3].data_ptr<float>()

// The tensor's device made current and torch's current stream on it.  A backward runs on autograd's worker thread: it
// sets the device and fetches the stream again.
struct OnDevice {
    c10::hip::HIPGuardMasqueradingAsCUDA guard;
    hipStream_t st;
    explicit OnDevice(const Tensor& t)
        : guard(t.device()), st(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream()) {}
};

// The head of every forward: the input as the kernels take it (cut from the graph, widened when it is no I/O type,
// contiguous, aligned), its device and stream, and per layer the caller's descriptor held to the tensor and the four
// coefficient views.  MultiFn has several layers on one input and calls layer() for each.
struct Prologue {
    Tensor u;
    OnDevice dev;
    PdeAdiDesc d;
    Tensor p[4];
    static Tensor input(const Tensor& u_in) {
        Tensor u = u_in.detach();
        if (!io_type(u)) u = u.to(at::kFloat);
        return aligned(u.contiguous());
    }
    explicit Prologue(const Tensor& u_in) : u(input(u_in)), dev(u) {}
    Prologue(const Tensor& u_in, const Tensor& ab, const Tensor& bb, const Tensor& asl, const Tensor& bsl, int64_t desc_addr)
        : Prologue(u_in) {
        layer(desc_addr, ab, bb, asl, bsl, &d, p);
    }
    void layer(int64_t desc_addr, const Tensor& ab, const Tensor& bb, const Tensor& asl, const Tensor& bsl, PdeAdiDesc* dd,
               Tensor* pp) const {
        std::memcpy(dd, reinterpret_cast<const void*>(desc_addr), sizeof(*dd));
        const int64_t C = u.size(1), N = u.size(2);
        PDE_REQUIRE(dd->B == u.size(0) && dd->C == C && dd->N == N && dd->io_dtype == io_of(u),
                    "descriptor does not match the tensor");
        pp[0] = as_chw(ab, C, N);
        pp[1] = as_chw(bb, C, N);
        pp[2] = as_chw(asl, C, N);
        pp[3] = as_chw(bsl, C, N);
    }
};

// A forward's request for its per-sweep coefficient maxima: the device buffer, a pinned slot with its event, and (unless
// the caller owns the slot: adi_lagged) the ticket that hands the slot back when the node dies.  All NULL when not wanted.
struct Kmax {
    Tensor kdev, ticket;
    Slot* slot = nullptr;
    Kmax(bool want, int n, const Tensor& u, bool own_ticket = true) {
        if (!want) return;
        kdev = at::empty({(int64_t)n}, u.options().dtype(at::kFloat));
        slot = acquire_slot(u.device().index());
        if (own_ticket) ticket = slot_ticket(slot, n);
    }
    float* dev() const { return fptr(kdev); }
    float* host() const { return slot ? slot->host : nullptr; }
    void* event() const { return slot ? (void*)slot->ev : nullptr; }
    void save(AutogradContext* ctx) const {
        if (ticket.defined()) {
            ctx->saved_data["ticket"] = ticket;
            ctx->saved_data["slot"] = (int64_t) reinterpret_cast<intptr_t>(slot);
        }
        if (kdev.defined()) ctx->saved_data["kdev"] = kdev;       // (the device copy lives as long as the node)
    }
};

// the union over the steps of the step-local plans (functional._plan_steps); one step of all sweeps is plan_checkpoints
void plan_steps(const float* kmax, int K, int sps, double amax, uint64_t mask[2]) {
    mask[0] = mask[1] = 0;
    for (int k = 0; k < K; ++k) {
        uint64_t m[2];
        plan_checkpoints(kmax + (size_t)k * sps, sps, amax, m);
        mask[0] |= m[0];
        mask[1] |= m[1];
    }
}

// ckpt_mode 1 = "auto": the backward plans from this call's coefficients; otherwise the mask is explicit
void save_plan(AutogradContext* ctx, int64_t ckpt_mode, int64_t lo, int64_t hi, double amax) {
    ctx->saved_data["ckpt"] = std::vector<int64_t>{ckpt_mode, lo, hi};
    ctx->saved_data["amax"] = amax;
}

// The backward's checkpoint mask: the explicit one, or under "auto" the plan — per step of `sps` sweeps — from the maxima
// in the node's slot, once the event behind the forward's factorisation kernel has completed.
void mask_from_ctx(AutogradContext* ctx, const PdeAdiDesc& d, int sps, uint64_t mask[2]) {
    auto ck = ctx->saved_data["ckpt"].toIntVector();
    mask[0] = (uint64_t)ck[1];
    mask[1] = (uint64_t)ck[2];
    if (ck[0] != 1) return;
    Slot* slot = reinterpret_cast<Slot*>((intptr_t)ctx->saved_data["slot"].toInt());
    wait_event(slot->ev);
    plan_steps(slot->host, d.num_sweeps / sps, sps, ctx->saved_data["amax"].toDouble(), mask);
}

void save_desc(AutogradContext* ctx, const PdeAdiDesc* d, int n = 1) {
    ctx->saved_data["desc"] = std::string(reinterpret_cast<const char*>(d), sizeof(PdeAdiDesc) * n);
}
void load_desc(AutogradContext* ctx, PdeAdiDesc* d, int n = 1) {
    std::memcpy(d, ctx->saved_data["desc"].toStringRef().data(), sizeof(PdeAdiDesc) * n);
}

// the callers' shapes of the four coefficient tensors of layer `i` — (N,N) at C = 1 — in which their gradients go back
void save_shapes(AutogradContext* ctx, std::initializer_list<const Tensor*> params, int i = 0) {
    int j = 4 * i;
    for (const Tensor* t : params) ctx->saved_data["sh" + std::to_string(j++)] = t->sizes().vec();
}
void param_grads(AutogradContext* ctx, const Tensor* p, Tensor* gp, int i = 0) {
    for (int j = 0; j < 4; ++j) gp[j] = at::empty(ctx->saved_data["sh" + std::to_string(4 * i + j)].toIntVector(), p[j].options());
}

// a cotangent as the library takes it: in the tensors' type, contiguous, aligned; an undefined one stays undefined
Tensor cotangent(Tensor g, at::ScalarType dtype) {
    if (!g.defined()) return g;
    if (g.scalar_type() != dtype) g = g.to(dtype);
    return aligned(g.contiguous());
}
Tensor as_dtype(const Tensor& g, int64_t dtype) {
    return (int64_t)g.scalar_type() == dtype ? g : g.to((at::ScalarType)dtype);
}

// the frozen route marks its node with the tensors' type (the node keeps no tensor of that type)
void save_input_only(AutogradContext* ctx, const Tensor& u) { ctx->saved_data["input_only"] = (int64_t)u.scalar_type(); }
bool is_input_only(AutogradContext* ctx) { return ctx->saved_data.count("input_only") != 0; }
at::ScalarType input_only_dtype(AutogradContext* ctx) {
    return static_cast<at::ScalarType>(ctx->saved_data["input_only"].toInt());
}

// a backward's result: the gradients it has, then undefined tensors up to the forward's `n` arguments
variable_list grads_out(size_t n, std::initializer_list<Tensor> head) {
    variable_list res(head);
    res.resize(n);
    return res;
}

// wide: a tensor or matrix the kernels read 16 bytes wide; otherwise one of the header's ELEMENT-ALIGNED parameters
// (skip_weight, weights, gamma / beta, bn_weight / bn_bias), which may begin wherever its elements do: no copy
Tensor as_f32(const Tensor& t, bool wide = true) {
    Tensor q = t.detach();
    if (q.scalar_type() != at::kFloat) q = q.to(at::kFloat);
    return wide ? aligned(q.contiguous()) : q.contiguous();
}

std::vector<int64_t> states_shape(int64_t K, const Tensor& u) {
    std::vector<int64_t> sh{K};
    for (auto v : u.sizes()) sh.push_back(v);
    return sh;
}

// ---- second order (functional.linear_adjoint): every node below is linear in its input, so its backward output is
// gu = F(theta)^T g and, for a cotangent v on gu, <v, F^T g> = <F v, g>: the gradient with respect to g is the node's own
// apply at v, the gradient with respect to theta the parameter gradient of that call with cotangent g.  A backward that runs
// in grad mode (create_graph=True) goes through AdjointFn (behind the nodes) and otherwise runs as it always has.  For that
// a node keeps its original parameter tensors — inputs, no copy — next to what it keeps anyway.
constexpr int64_t kAdi = 0, kSmall = 1, kMixed = 2, kMulti = 3;
variable_list second_order(int64_t kind, AutogradContext* outer, const variable_list& grads);
void save_orig(AutogradContext* ctx, std::initializer_list<const Tensor*> params) {
    std::vector<Tensor> v;
    for (const Tensor* t : params)
        if (t->defined()) v.push_back(*t);
    ctx->saved_data["orig"] = v;
}

// The nodes that are NOT linear in their input (the symmetric layers) are differentiable once: what
// torch.autograd.function.once_differentiable does for their ctypes twins — in grad mode, with a cotangent that requires
// grad, the results carry a node that raises when it is differentiated, instead of passing for constants.
variable_list once_differentiable(const variable_list& grads, variable_list outs) {
    bool twice = false;
    if (at::GradMode::is_enabled())
        for (const auto& g : grads) twice = twice || (g.defined() && g.requires_grad());
    if (!twice) return outs;
    variable_list in;
    std::vector<size_t> pos;
    for (size_t i = 0; i < outs.size(); ++i)
        if (outs[i].defined()) {
            Tensor t = outs[i].detach();
            t.set_requires_grad(true);
            in.push_back(t);
            pos.push_back(i);
        }
    auto err = std::make_shared<torch::autograd::DelayedError>(
        "trying to differentiate twice a function that is differentiable once (the symmetric layer is not linear in its "
        "input: second order is not supported)", (int64_t)in.size());
    variable_list res = (*err)(std::move(in));
    for (size_t k = 0; k < pos.size(); ++k) outs[pos[k]] = res[k];
    return outs;
}

struct AdiFn : public torch::autograd::Function<AdiFn> {
    // ckpt_mode: 0 = explicit mask (ckpt_lo/hi), 1 = "auto" (planned in the backward from this call's coefficients),
    // 2 = explicit mask, and this call's coefficient maxima go to a slot the CALLER owns (slot_out: where to leave it) —
    // the "lagged" policy of layers.py: the next call plans from them, nobody waits
    static Tensor forward(AutogradContext* ctx, const Tensor& u_in, const Tensor& ab, const Tensor& bb, const Tensor& asl,
                          const Tensor& bsl, int64_t desc_addr, int64_t ckpt_mode, int64_t ckpt_lo, int64_t ckpt_hi,
                          double amax, int64_t grad_mode, int64_t slot_out) {
        const bool need_grad = grad_mode != kGradNone, input_only = grad_mode == kGradInput;
        require_cuda({&u_in, &ab, &bb, &asl, &bsl});
        PDE_REQUIRE(u_in.dim() == 4 && u_in.size(2) == u_in.size(3), "expected (B,C,N,N), got ", u_in.sizes());
        Prologue pr(u_in, ab, bb, asl, bsl, desc_addr);
        const Tensor& u = pr.u;
        const PdeAdiDesc& d = pr.d;
        Tensor y = at::empty_like(u);
        Tensor ws = bytes(pde_adi_forward_workspace_bytes(&d), u);
        // (the input-only backward plans no checkpoints: maxima only for the lagged call, which hands the ticket out)
        Kmax km(need_grad && (ckpt_mode == 2 || (ckpt_mode == 1 && !input_only)), d.num_sweeps, u, ckpt_mode == 1);
        if (km.slot && ckpt_mode != 1) *reinterpret_cast<Slot**>(slot_out) = km.slot;   // the caller's ticket holds it
        check(pde_adi_forward(&d, u.data_ptr(), y.data_ptr(), PDE_F4(pr.p), km.dev(), km.host(), km.event(), ws.data_ptr(),
                              (size_t)ws.numel(), (void*)pr.dev.st),
              "pde_adi_forward");
        if (!need_grad) return y;
        if (input_only) {
            ctx->save_for_backward({pr.p[0], pr.p[1], pr.p[2], pr.p[3]});
            save_input_only(ctx, u);
        } else {
            const bool explicit_none = ckpt_mode == 0 && ckpt_lo == 0 && ckpt_hi == 0;
            ctx->save_for_backward({y, explicit_none ? Tensor() : u, pr.p[0], pr.p[1], pr.p[2], pr.p[3]});
            save_plan(ctx, ckpt_mode, ckpt_lo, ckpt_hi, amax);
            save_shapes(ctx, {&ab, &bb, &asl, &bsl});
        }
        ctx->saved_data["ws"] = ws;                          // the factorisation, reused by the backward
        km.save(ctx);
        save_desc(ctx, &d);
        save_orig(ctx, {&ab, &bb, &asl, &bsl});
        return y;
    }

    // gu = F^T gy alone: the coefficient views, the forward's factorisation, one launch
    static variable_list backward_input(AutogradContext* ctx, variable_list& grads) {
        auto saved = ctx->get_saved_variables();
        PdeAdiDesc d;
        load_desc(ctx, &d);
        Tensor gy = cotangent(grads[0], input_only_dtype(ctx));
        OnDevice dev(gy);
        Tensor gu = at::empty_like(gy);
        Tensor ws = bytes(pde_adi_backward_input_workspace_bytes(&d), gy);
        Tensor fws = ctx->saved_data["ws"].toTensor();
        check(pde_adi_backward_input(&d, gy.data_ptr(), gu.data_ptr(), PDE_F4(&saved[0]), fws.data_ptr(), ws.data_ptr(),
                                     (size_t)ws.numel(), (void*)dev.st),
              "pde_adi_backward_input");
        return grads_out(12, {gu});
    }

    static variable_list backward(AutogradContext* ctx, variable_list grads) {
        if (at::GradMode::is_enabled()) return second_order(kAdi, ctx, grads);   // create_graph=True
        return backward_now(ctx, grads);
    }

    static variable_list backward_now(AutogradContext* ctx, variable_list& grads) {
        if (is_input_only(ctx)) return backward_input(ctx, grads);
        auto saved = ctx->get_saved_variables();
        const Tensor &y = saved[0], &u = saved[1];
        PdeAdiDesc d;
        load_desc(ctx, &d);
        uint64_t mask[2];
        mask_from_ctx(ctx, d, d.num_sweeps, mask);
        const bool any = (mask[0] | mask[1]) != 0;
        PDE_REQUIRE(!any || u.defined(), "a checkpoint plan needs the layer input, which was not kept");
        OnDevice dev(y);
        Tensor gy = cotangent(grads[0], y.scalar_type());
        Tensor gu = at::empty_like(y);
        Tensor gp[4];
        param_grads(ctx, &saved[2], gp);
        Tensor ws = bytes(pde_adi_backward_workspace_bytes(&d, popcount2(mask)), y);
        Tensor fws = ctx->saved_data["ws"].toTensor();
        check(pde_adi_backward(&d, gy.data_ptr(), y.data_ptr(), any ? u.data_ptr() : nullptr, mask, gu.data_ptr(),
                               PDE_F4(&saved[2]), PDE_F4(gp), fws.data_ptr(), ws.data_ptr(), (size_t)ws.numel(), (void*)dev.st),
              "pde_adi_backward");
        return grads_out(12, {gu, gp[0], gp[1], gp[2], gp[3]});
    }
};

Tensor adi(const Tensor& u, const Tensor& ab, const Tensor& bb, const Tensor& asl, const Tensor& bsl, int64_t desc_addr,
           int64_t ckpt_mode, int64_t ckpt_lo, int64_t ckpt_hi, double amax) {
    // forward() runs with grad mode off: whether anything is kept for a backward, and what, is decided out here
    return AdiFn::apply(u, ab, bb, asl, bsl, desc_addr, ckpt_mode, ckpt_lo, ckpt_hi, amax, adi_grad_mode(u, ab, bb, asl, bsl),
                        (int64_t)0);
}

// The coefficient maxima of one call, for whoever plans a LATER call from them (layers.py, "lagged" policy): `event`
// / `query()` / `host` as the ctypes path's tickets have them.  Holds its pinned slot until it is dropped.
struct Ticket {
    Slot* slot;
    int n;
    Ticket(Slot* s, int n_) : slot(s), n(n_) {}
    Ticket(const Ticket&) = delete;
    ~Ticket() { release_slot(slot); }
    bool query() const { return hipEventQuery(slot->ev) == hipSuccess; }
    void synchronize() const { wait_event(slot->ev); }
    Tensor host() const { return at::from_blob(slot->host, {n}, at::TensorOptions().dtype(at::kFloat)).clone(); }
};

std::pair<Tensor, std::shared_ptr<Ticket>> adi_lagged(const Tensor& u, const Tensor& ab, const Tensor& bb, const Tensor& asl,
                                                      const Tensor& bsl, int64_t desc_addr, int64_t ckpt_lo, int64_t ckpt_hi) {
    Slot* slot = nullptr;
    Tensor y = AdiFn::apply(u, ab, bb, asl, bsl, desc_addr, (int64_t)2, ckpt_lo, ckpt_hi, 0.0,
                            adi_grad_mode(u, ab, bb, asl, bsl), (int64_t) reinterpret_cast<intptr_t>(&slot));
    PdeAdiDesc d;
    std::memcpy(&d, reinterpret_cast<const void*>(desc_addr), sizeof(d));
    return {y, slot ? std::make_shared<Ticket>(slot, d.num_sweeps) : std::shared_ptr<Ticket>()};
}

// ---- one layer with a channel operator between its steps, C <= 4, one launch per pass (functional._AdiSmallFn without
// ``emit``: cifar10.py:84-112 "pre", SVHN.py:55-76 "post" with the skip blend) ---------------------------------------
struct SmallFn : public torch::autograd::Function<SmallFn> {
    static Tensor forward(AutogradContext* ctx, const Tensor& u_in, const Tensor& ab, const Tensor& bb, const Tensor& asl,
                          const Tensor& bsl, const Tensor& M, const std::optional<Tensor>& skip_opt, int64_t desc_addr, int64_t sps,
                          int64_t mode, int64_t ckpt_mode, int64_t ckpt_lo, double amax, int64_t grad_mode) {
        // kGradInput: frozen parameters — pde_adi_small_forward_input parks nothing, and the backward is
        // pde_adi_small_backward_input (M, skip_weight and the steps workspace are all it keeps)
        const bool need_grad = grad_mode == kGradFull, input_only = grad_mode == kGradInput;
        const Tensor skip = skip_opt.has_value() ? *skip_opt : Tensor();
        require_cuda({&u_in, &ab, &bb, &asl, &bsl, &M, &skip});
        Prologue pr(u_in, ab, bb, asl, bsl, desc_addr);
        const Tensor& u = pr.u;
        const PdeAdiDesc& d = pr.d;
        Tensor Mf = as_f32(M);
        Tensor sw = skip.defined() ? as_f32(skip, false).reshape({1}) : Tensor();
        Tensor sws = bytes(pde_adi_steps_workspace_bytes(&d, (int32_t)sps), u);
        Kmax km(need_grad && ckpt_mode == 1, d.num_sweeps, u);
        Tensor states = need_grad ? at::empty(states_shape(d.num_sweeps / sps, u), u.options()) : Tensor();
        Tensor y = at::empty_like(u);
        if (input_only)
            check(pde_adi_small_forward_input(&d, (int32_t)sps, (int32_t)mode, u.data_ptr(), y.data_ptr(), Mf.data_ptr<float>(),
                                              fptr(sw), PDE_F4(pr.p), nullptr, nullptr, nullptr, sws.data_ptr(),
                                              (size_t)sws.numel(), (void*)pr.dev.st),
                  "pde_adi_small_forward_input");
        else
            check(pde_adi_small_forward(&d, (int32_t)sps, (int32_t)mode, u.data_ptr(), y.data_ptr(), vptr(states),
                                        Mf.data_ptr<float>(), fptr(sw), PDE_F4(pr.p), km.dev(), km.host(), km.event(),
                                        sws.data_ptr(), (size_t)sws.numel(), (void*)pr.dev.st),
                  "pde_adi_small_forward");
        if (grad_mode == kGradNone) return y;
        if (input_only) {
            ctx->save_for_backward({Mf, sw});
            save_input_only(ctx, u);
        } else {
            ctx->save_for_backward({u, Mf, sw, pr.p[0], pr.p[1], pr.p[2], pr.p[3]});
            ctx->saved_data["states"] = states;
            km.save(ctx);
            save_plan(ctx, ckpt_mode, ckpt_lo, 0, amax);
            save_shapes(ctx, {&ab, &bb, &asl, &bsl});
            ctx->saved_data["types"] = std::vector<int64_t>{(int64_t)M.scalar_type(),
                                                            skip.defined() ? (int64_t)skip.scalar_type() : -1};
            if (skip.defined()) ctx->saved_data["shs"] = skip.sizes().vec();
        }
        ctx->saved_data["sws"] = sws;
        save_desc(ctx, &d);
        ctx->saved_data["cfg"] = std::vector<int64_t>{sps, mode};
        save_orig(ctx, {&ab, &bb, &asl, &bsl, &M, &skip});
        return y;
    }

    // gu = F^T gy alone: the operator, the skip weight, the forward's factorisation, one launch
    static variable_list backward_input(AutogradContext* ctx, variable_list& grads) {
        auto saved = ctx->get_saved_variables();
        const Tensor &Mf = saved[0], &sw = saved[1];
        PdeAdiDesc d;
        load_desc(ctx, &d);
        auto cfg = ctx->saved_data["cfg"].toIntVector();
        Tensor gy = cotangent(grads[0], input_only_dtype(ctx));
        OnDevice dev(gy);
        Tensor gu = at::empty_like(gy);
        Tensor sws = ctx->saved_data["sws"].toTensor();
        check(pde_adi_small_backward_input(&d, (int32_t)cfg[0], (int32_t)cfg[1], gy.data_ptr(), Mf.data_ptr<float>(), fptr(sw),
                                           gu.data_ptr(), sws.data_ptr(), nullptr, 0, (void*)dev.st),
              "pde_adi_small_backward_input");
        return grads_out(14, {gu});
    }

    static variable_list backward(AutogradContext* ctx, variable_list grads) {
        if (at::GradMode::is_enabled()) return second_order(kSmall, ctx, grads);   // create_graph=True
        return backward_now(ctx, grads);
    }

    static variable_list backward_now(AutogradContext* ctx, variable_list& grads) {
        if (is_input_only(ctx)) return backward_input(ctx, grads);
        auto saved = ctx->get_saved_variables();
        const Tensor &u = saved[0], &Mf = saved[1], &sw = saved[2];
        PdeAdiDesc d;
        load_desc(ctx, &d);
        auto cfg = ctx->saved_data["cfg"].toIntVector();
        auto types = ctx->saved_data["types"].toIntVector();
        const int sps = (int)cfg[0], mode = (int)cfg[1];
        uint64_t mask[2];
        mask_from_ctx(ctx, d, sps, mask);
        OnDevice dev(u);
        Tensor gy = cotangent(grads[0], u.scalar_type());
        Tensor gu = at::empty_like(gy);
        Tensor gp[4];
        param_grads(ctx, &saved[3], gp);
        Tensor gM = at::empty_like(Mf);
        Tensor gsw = sw.defined() ? at::empty({1}, Mf.options()) : Tensor();
        Tensor ws = bytes(pde_adi_small_backward_workspace_bytes(&d, sps, popcount2(mask)), u);
        Tensor states = ctx->saved_data["states"].toTensor(), sws = ctx->saved_data["sws"].toTensor();
        check(pde_adi_small_backward(&d, sps, mode, gy.data_ptr(), u.data_ptr(), states.data_ptr(), Mf.data_ptr<float>(), fptr(sw),
                                     mask, gu.data_ptr(), PDE_F4(&saved[3]), PDE_F4(gp), gM.data_ptr<float>(), fptr(gsw),
                                     sws.data_ptr(), ws.data_ptr(), (size_t)ws.numel(), (void*)dev.st),
              "pde_adi_small_backward");
        if (gsw.defined()) gsw = as_dtype(gsw, types[1]).reshape(ctx->saved_data["shs"].toIntVector());
        return grads_out(14, {gu, gp[0], gp[1], gp[2], gp[3], as_dtype(gM, types[0]), gsw});
    }
};

Tensor small(const Tensor& u, const Tensor& ab, const Tensor& bb, const Tensor& asl, const Tensor& bsl, const Tensor& M,
             const std::optional<Tensor>& skip, int64_t desc_addr, int64_t sps, int64_t mode, int64_t ckpt_mode, int64_t ckpt_lo,
             double amax) {
    const Tensor sk = (skip.has_value() && skip->defined()) ? *skip : Tensor();
    const std::optional<Tensor> sko = sk.defined() ? std::optional<Tensor>(sk) : std::nullopt;
    const bool params = ab.requires_grad() || bb.requires_grad() || asl.requires_grad() || bsl.requires_grad() ||
                        M.requires_grad() || (sk.defined() && sk.requires_grad());
    return SmallFn::apply(u, ab, bb, asl, bsl, M, sko, desc_addr, sps, mode, ckpt_mode, ckpt_lo, amax, grad_mode_of(u, params));
}

// ---- one layer with a channel operator between its steps at any width: one factorisation, then per step one mixing and
// one sweep launch (or the whole forward in one launch at C = 32 / 64), looped inside the library
// (functional._AdiMixedFn: cifar10.py:84-112 "pre", SVHN.py:55-72 "post") -------------------------------------------------
struct MixedFn : public torch::autograd::Function<MixedFn> {
    static Tensor forward(AutogradContext* ctx, const Tensor& u_in, const Tensor& ab, const Tensor& bb, const Tensor& asl,
                          const Tensor& bsl, const Tensor& M, int64_t desc_addr, int64_t sps, int64_t mode, int64_t ckpt_mode,
                          int64_t ckpt_lo, double amax, int64_t grad_mode) {
        // kGradInput (frozen parameters) and kGradNone: pde_adi_mixed_forward_input keeps no state at all, and the backward
        // of the former is pde_adi_mixed_backward_input (M and the steps workspace are all it keeps).  PDE_BWD_INPUT=0
        // restores pde_adi_mixed_forward for both.
        const bool need_grad = grad_mode == kGradFull;
        require_cuda({&u_in, &ab, &bb, &asl, &bsl, &M});
        PDE_REQUIRE(u_in.dim() == 4 && u_in.size(2) == u_in.size(3), "expected (B,C,N,N), got ", u_in.sizes());
        Prologue pr(u_in, ab, bb, asl, bsl, desc_addr);
        const Tensor& u = pr.u;
        const PdeAdiDesc& d = pr.d;
        Tensor Mf = as_f32(M);
        Tensor sws = bytes(pde_adi_steps_workspace_bytes(&d, (int32_t)sps), u);
        if (!need_grad && bwd_input_enabled()) {
            Tensor y = at::empty_like(u);
            Tensor ws = bytes(pde_adi_mixed_forward_input_workspace_bytes(&d, (int32_t)sps), u);
            check(pde_adi_mixed_forward_input(&d, (int32_t)sps, (int32_t)mode, u.data_ptr(), y.data_ptr(), Mf.data_ptr<float>(),
                                              PDE_F4(pr.p), nullptr, nullptr, nullptr, sws.data_ptr(), (size_t)sws.numel(),
                                              ws.data_ptr(), (size_t)ws.numel(), (void*)pr.dev.st),
                  "pde_adi_mixed_forward_input");
            if (grad_mode == kGradNone) return y;
            ctx->save_for_backward({Mf});
            save_input_only(ctx, u);
            ctx->saved_data["sws"] = sws;
            save_desc(ctx, &d);
            ctx->saved_data["cfg"] = std::vector<int64_t>{sps, mode, (int64_t)M.scalar_type()};
            save_orig(ctx, {&ab, &bb, &asl, &bsl, &M});
            return y;
        }
        Kmax km(need_grad && ckpt_mode == 1, d.num_sweeps, u);
        // states[2k]: output of step k's first operator, states[2k+1]: of its second (= input of step k + 1); the last of
        // them is the layer output and lives in a tensor of its own
        Tensor states = at::empty(states_shape(2 * (d.num_sweeps / sps) - 1, u), u.options());
        Tensor y = at::empty_like(u);
        check(pde_adi_mixed_forward(&d, (int32_t)sps, (int32_t)mode, u.data_ptr(), states.data_ptr(), y.data_ptr(),
                                    Mf.data_ptr<float>(), PDE_F4(pr.p), km.dev(), km.host(), km.event(), sws.data_ptr(),
                                    (size_t)sws.numel(), (void*)pr.dev.st),
              "pde_adi_mixed_forward");
        if (grad_mode == kGradNone) return y;
        ctx->save_for_backward({u, states, Mf, pr.p[0], pr.p[1], pr.p[2], pr.p[3], y});
        ctx->saved_data["sws"] = sws;
        km.save(ctx);
        save_desc(ctx, &d);
        save_plan(ctx, ckpt_mode, ckpt_lo, 0, amax);
        save_shapes(ctx, {&ab, &bb, &asl, &bsl});
        ctx->saved_data["cfg"] = std::vector<int64_t>{sps, mode, (int64_t)M.scalar_type()};
        save_orig(ctx, {&ab, &bb, &asl, &bsl, &M});
        return y;
    }

    // gu = F^T gy alone: the operator and the forward's factorisation, per step M^T g and the transposed solves
    static variable_list backward_input(AutogradContext* ctx, variable_list& grads) {
        auto saved = ctx->get_saved_variables();
        const Tensor& Mf = saved[0];
        PdeAdiDesc d;
        load_desc(ctx, &d);
        auto cfg = ctx->saved_data["cfg"].toIntVector();
        Tensor gy = cotangent(grads[0], input_only_dtype(ctx));
        OnDevice dev(gy);
        Tensor gu = at::empty_like(gy);
        Tensor sws = ctx->saved_data["sws"].toTensor();
        Tensor ws = bytes(pde_adi_mixed_backward_input_workspace_bytes(&d, (int32_t)cfg[0]), gy);
        check(pde_adi_mixed_backward_input(&d, (int32_t)cfg[0], (int32_t)cfg[1], gy.data_ptr(), Mf.data_ptr<float>(),
                                           gu.data_ptr(), sws.data_ptr(), ws.data_ptr(), (size_t)ws.numel(), (void*)dev.st),
              "pde_adi_mixed_backward_input");
        return grads_out(13, {gu});
    }

    static variable_list backward(AutogradContext* ctx, variable_list grads) {
        if (at::GradMode::is_enabled()) return second_order(kMixed, ctx, grads);   // create_graph=True
        return backward_now(ctx, grads);
    }

    static variable_list backward_now(AutogradContext* ctx, variable_list& grads) {
        if (is_input_only(ctx)) return backward_input(ctx, grads);
        auto saved = ctx->get_saved_variables();
        const Tensor &u = saved[0], &states = saved[1], &Mf = saved[2];
        PdeAdiDesc d;
        load_desc(ctx, &d);
        auto cfg = ctx->saved_data["cfg"].toIntVector();
        const int sps = (int)cfg[0], mode = (int)cfg[1];
        uint64_t mask[2];
        mask_from_ctx(ctx, d, sps, mask);
        OnDevice dev(u);
        Tensor gy = cotangent(grads[0], u.scalar_type());
        Tensor gu = at::empty_like(gy);
        Tensor gp[4];
        param_grads(ctx, &saved[3], gp);
        Tensor gM = at::empty_like(Mf);
        Tensor ws = bytes(pde_adi_mixed_backward_workspace_bytes(&d, sps, popcount2(mask)), u);
        Tensor sws = ctx->saved_data["sws"].toTensor();
        check(pde_adi_mixed_backward(&d, sps, mode, gy.data_ptr(), u.data_ptr(), states.data_ptr(), saved[7].data_ptr(),
                                     Mf.data_ptr<float>(), mask, gu.data_ptr(), PDE_F4(&saved[3]), PDE_F4(gp),
                                     gM.data_ptr<float>(), sws.data_ptr(), ws.data_ptr(), (size_t)ws.numel(), (void*)dev.st),
              "pde_adi_mixed_backward");
        return grads_out(13, {gu, gp[0], gp[1], gp[2], gp[3], as_dtype(gM, cfg[2])});
    }
};

Tensor mixed(const Tensor& u, const Tensor& ab, const Tensor& bb, const Tensor& asl, const Tensor& bsl, const Tensor& M,
             int64_t desc_addr, int64_t sps, int64_t mode, int64_t ckpt_mode, int64_t ckpt_lo, double amax) {
    const bool params = ab.requires_grad() || bb.requires_grad() || asl.requires_grad() || bsl.requires_grad() || M.requires_grad();
    return MixedFn::apply(u, ab, bb, asl, bsl, M, desc_addr, sps, mode, ckpt_mode, ckpt_lo, amax, grad_mode_of(u, params));
}

// ---- several mixing-first layers on the SAME input, one launch per pass (functional._AdiMultiFn: cifar10.py:272-280,
// cifar_2version.py:287-288).  Returns (sum_i w_i y_i, y_1 .. y_L[, s_1 .. s_L]) ----------------------------------------
struct MultiFn : public torch::autograd::Function<MultiFn> {
    // what every pass sets of a layer's record (functional._small_layer); the caller adds what its pass has
    static PdeSmallLayer layer_record(const PdeAdiDesc* d, int64_t sps, const Tensor& Mf, const Tensor& wdev, int i,
                                      const Tensor& sws) {
        PdeSmallLayer a;
        std::memset(&a, 0, sizeof(a));
        a.desc = d;
        a.sweeps_per_step = (int32_t)sps;
        a.mode = 1;
        a.M = Mf.data_ptr<float>();
        a.weight = 0.f;
        a.weight_ptr = wdev.defined() ? wdev.data_ptr<float>() + i : nullptr;
        a.steps_workspace = sws.data_ptr();
        a.steps_workspace_bytes = (size_t)sws.numel();
        return a;
    }
    static void set_coeffs(PdeSmallLayer& a, const Tensor* p) {
        a.alpha_base = p[0].data_ptr<float>();
        a.beta_base = p[1].data_ptr<float>();
        a.alpha_slope = p[2].data_ptr<float>();
        a.beta_slope = p[3].data_ptr<float>();
    }
    // the cotangents of layer `i` (its y_i and, with plane sums, its s_i) into its record; false when it has neither
    static bool set_cotangents(PdeSmallLayer& a, const variable_list& grads, int i, int nl, bool want_sums,
                               at::ScalarType dtype, std::vector<Tensor>& keep) {
        Tensor gyi = cotangent(grads[1 + i], dtype);
        Tensor gsi = want_sums ? cotangent(grads[1 + nl + i], at::kFloat) : Tensor();
        a.gys = vptr(gyi);
        a.g_plane_sums = fptr(gsi);
        keep.push_back(gyi);
        keep.push_back(gsi);
        return gyi.defined() || gsi.defined();
    }

    static variable_list forward(AutogradContext* ctx, const Tensor& u_in, const std::optional<Tensor>& w_opt, at::TensorList flat,
                                 std::vector<int64_t> desc_addrs, int64_t sps, bool want_sums, int64_t ckpt_mode,
                                 std::vector<int64_t> masks, double amax, int64_t grad_mode) {
        // kGradInput: frozen parameters — the forward is the same call (the y_i are the last kept states), but no
        // coefficient maxima are asked for and the node keeps the operators, the weights and the factorisations only
        const bool need_grad = grad_mode != kGradNone, input_only = grad_mode == kGradInput;
        const int nl = (int)desc_addrs.size();
        const Tensor weights = w_opt.has_value() ? *w_opt : Tensor();
        PDE_REQUIRE(nl >= 1 && (int)flat.size() == 5 * nl, "adi_diffuse_multi: five tensors per layer");
        require_cuda({&u_in, &weights});
        for (const auto& t : flat) require_cuda({&t});
        Prologue pr(u_in);
        const Tensor& u = pr.u;
        const bool want_kmax = need_grad && ckpt_mode == 1 && !input_only;
        ctx->set_materialize_grads(false);
        Tensor wdev = weights.defined() ? as_f32(weights, false) : Tensor();

        std::vector<PdeAdiDesc> descs(nl);
        std::vector<PdeSmallLayer> arr(nl);
        std::vector<Tensor> save, views, hold, states_v, sums_v, tickets;
        if (!input_only) save.push_back(u);
        save.push_back(wdev);
        std::vector<int64_t> slots, mdt;
        for (int i = 0; i < nl; ++i) {
            PdeAdiDesc& d = descs[i];
            Tensor p[4];
            pr.layer(desc_addrs[i], flat[5 * i], flat[5 * i + 1], flat[5 * i + 2], flat[5 * i + 3], &d, p);
            Tensor Mf = as_f32(flat[5 * i + 4]);
            Tensor sws = bytes(pde_adi_steps_workspace_bytes(&d, (int32_t)sps), u);
            Tensor states = at::empty(states_shape(d.num_sweeps / sps, u), u.options());
            Kmax km(want_kmax, d.num_sweeps, u);
            if (want_kmax) {
                tickets.push_back(km.ticket);
                hold.push_back(km.kdev);
            }
            slots.push_back((int64_t) reinterpret_cast<intptr_t>(km.slot));
            Tensor psum = want_sums ? at::empty({u.size(0), u.size(1)}, u.options().dtype(at::kFloat)) : Tensor();
            PdeSmallLayer& a = arr[i] = layer_record(&d, sps, Mf, wdev, i, sws);
            set_coeffs(a, p);
            a.states = states.data_ptr();
            a.kappa_max = km.dev();
            a.kappa_max_host = km.host();
            a.plane_sums = fptr(psum);
            // (the views may be fp32 copies of 16-bit parameters: alive until the launch on every route)
            for (int j = 0; j < 4; ++j) (input_only ? views : save).push_back(p[j]);
            save.push_back(Mf);
            hold.push_back(sws);
            states_v.push_back(states);
            sums_v.push_back(psum);
            mdt.push_back((int64_t)flat[5 * i + 4].scalar_type());
            if (need_grad && !input_only) save_shapes(ctx, {&flat[5 * i], &flat[5 * i + 1], &flat[5 * i + 2], &flat[5 * i + 3]}, i);
        }
        Tensor out = at::empty_like(u);
        Slot* last = want_kmax ? reinterpret_cast<Slot*>((intptr_t)slots.back()) : nullptr;   // recorded behind the last layer's copy
        check(pde_adi_multi_forward(nl, arr.data(), u.data_ptr(), out.data_ptr(), last ? (void*)last->ev : nullptr,
                                    (void*)pr.dev.st),
              "pde_adi_multi_forward");
        if (need_grad) {
            // frozen: the weights and the operators; else the input, the weights, per layer four views and the operator
            ctx->save_for_backward(save);
            ctx->saved_data["hold"] = hold;                   // per layer [kdev with coefficient maxima,] the steps workspace
            save_desc(ctx, descs.data(), nl);
            ctx->saved_data["cfg"] = std::vector<int64_t>{nl, sps, want_sums ? 1 : 0, ckpt_mode, weights.defined() ? 1 : 0};
            {
                std::vector<Tensor> orig(flat.begin(), flat.end());             // the five tensors per layer, then the weights
                if (weights.defined()) orig.push_back(weights);
                ctx->saved_data["orig"] = orig;
            }
            if (input_only) {
                save_input_only(ctx, u);
                ctx->saved_data["ushape"] = u.sizes().vec();
            } else {
                ctx->saved_data["states"] = states_v;
                if (want_kmax) ctx->saved_data["tickets"] = tickets;
                ctx->saved_data["slots"] = slots;
                ctx->saved_data["masks"] = masks;
                ctx->saved_data["mdt"] = mdt;
                ctx->saved_data["amax"] = amax;
            }
        }
        variable_list res{out};
        for (int i = 0; i < nl; ++i) res.push_back(states_v[i].select(0, states_v[i].size(0) - 1));   // the last sweep output of every layer
        if (want_sums)
            for (int i = 0; i < nl; ++i) res.push_back(sums_v[i]);
        return res;
    }

    // gu = sum_i F_i^T (w_i gy + gys_i + g_plane_sums_i) alone: pde_adi_multi_backward_input, one launch (two side by side)
    static variable_list backward_input(AutogradContext* ctx, variable_list& grads) {
        auto saved = ctx->get_saved_variables();
        auto cfg = ctx->saved_data["cfg"].toIntVector();
        const int nl = (int)cfg[0], sps = (int)cfg[1];
        const Tensor& wdev = saved[0];
        const auto dtype = input_only_dtype(ctx);
        std::vector<PdeAdiDesc> descs(nl);
        load_desc(ctx, descs.data(), nl);
        auto hold = ctx->saved_data["hold"].toTensorVector();
        const Tensor& like = saved[1];
        OnDevice dev(like);
        Tensor gout = cotangent(grads[0], dtype);
        std::vector<PdeSmallLayer> arr(nl);
        std::vector<Tensor> keep;
        bool any_in = gout.defined();
        for (int i = 0; i < nl; ++i) {
            PdeSmallLayer& a = arr[i] = layer_record(&descs[i], sps, saved[1 + i], wdev, i, hold[i]);
            any_in = set_cotangents(a, grads, i, nl, cfg[2] != 0, dtype, keep) || any_in;
            // (the slab of a side-by-side group; the query is what the library checks against, used or not)
            Tensor ws = nl > 1 ? bytes(pde_adi_small_backward_input_workspace_bytes(&descs[i], sps), like) : Tensor();
            a.workspace = vptr(ws);
            a.workspace_bytes = ws.defined() ? (size_t)ws.numel() : 0;
            keep.push_back(ws);
        }
        PDE_REQUIRE(any_in, "adi_diffuse_multi: no incoming gradient");
        Tensor gu = at::empty(ctx->saved_data["ushape"].toIntVector(), like.options().dtype(dtype));
        check(pde_adi_multi_backward_input(nl, arr.data(), vptr(gout), gu.data_ptr(), (void*)dev.st),
              "pde_adi_multi_backward_input");
        return grads_out(2 + 5 * nl + 7, {gu});
    }

    static variable_list backward(AutogradContext* ctx, variable_list grads) {
        if (at::GradMode::is_enabled()) return second_order(kMulti, ctx, grads);   // create_graph=True
        return backward_now(ctx, grads);
    }

    static variable_list backward_now(AutogradContext* ctx, variable_list& grads) {
        if (is_input_only(ctx)) return backward_input(ctx, grads);
        auto saved = ctx->get_saved_variables();
        auto cfg = ctx->saved_data["cfg"].toIntVector();
        const int nl = (int)cfg[0], sps = (int)cfg[1];
        const bool has_w = cfg[4] != 0, planned = cfg[3] == 1;
        const Tensor &u = saved[0], &wdev = saved[1];
        std::vector<PdeAdiDesc> descs(nl);
        load_desc(ctx, descs.data(), nl);
        auto slots = ctx->saved_data["slots"].toIntVector();
        auto masks = ctx->saved_data["masks"].toIntVector();
        auto mdt = ctx->saved_data["mdt"].toIntVector();
        auto states_v = ctx->saved_data["states"].toTensorVector();
        auto hold = ctx->saved_data["hold"].toTensorVector();
        const double amax = ctx->saved_data["amax"].toDouble();
        if (planned) wait_event(reinterpret_cast<Slot*>((intptr_t)slots.back())->ev);
        OnDevice dev(u);
        Tensor gout = cotangent(grads[0], u.scalar_type());
        std::vector<PdeSmallLayer> arr(nl);
        std::vector<uint64_t> mk(2 * nl);
        std::vector<Tensor> keep, gws;
        variable_list res(2 + 5 * nl + 7);                    // u, weights, five per layer, the seven non-tensor arguments
        bool any_in = gout.defined();
        for (int i = 0; i < nl; ++i) {
            PdeAdiDesc& d = descs[i];
            uint64_t* m = &mk[2 * i];
            m[0] = m[1] = 0;
            if (planned) plan_steps(reinterpret_cast<Slot*>((intptr_t)slots[i])->host, d.num_sweeps / sps, sps, amax, m);
            else m[0] = (uint64_t)masks[i];
            const Tensor* p = &saved[2 + 5 * i];
            const Tensor& Mf = saved[2 + 5 * i + 4];
            Tensor ws = bytes(pde_adi_small_backward_workspace_bytes(&d, sps, popcount2(m)), u);
            Tensor gp[4];
            param_grads(ctx, p, gp, i);
            Tensor gM = at::empty_like(Mf);
            Tensor gw = at::empty({1}, Mf.options());
            // hold: [kdev, sws] per layer with coefficient maxima, else [sws]
            PdeSmallLayer& a = arr[i] = layer_record(&d, sps, Mf, wdev, i, hold[planned ? 2 * i + 1 : i]);
            set_coeffs(a, p);
            any_in = set_cotangents(a, grads, i, nl, cfg[2] != 0, u.scalar_type(), keep) || any_in;
            a.states = states_v[i].data_ptr();
            a.ckpt_mask = m;
            a.g_alpha_base = gp[0].data_ptr<float>();
            a.g_beta_base = gp[1].data_ptr<float>();
            a.g_alpha_slope = gp[2].data_ptr<float>();
            a.g_beta_slope = gp[3].data_ptr<float>();
            a.gM = gM.data_ptr<float>();
            a.g_weight = gw.data_ptr<float>();
            a.workspace = ws.data_ptr();
            a.workspace_bytes = (size_t)ws.numel();
            keep.push_back(ws);
            for (int j = 0; j < 4; ++j) res[2 + 5 * i + j] = gp[j];
            res[2 + 5 * i + 4] = gM;                                        // converted to the operator's type behind the launch
            gws.push_back(gw);
        }
        PDE_REQUIRE(any_in, "adi_diffuse_multi: no incoming gradient");
        Tensor gu = at::empty_like(u);
        check(pde_adi_multi_backward(nl, arr.data(), vptr(gout), u.data_ptr(), gu.data_ptr(), (void*)dev.st),
              "pde_adi_multi_backward");
        for (int i = 0; i < nl; ++i) res[2 + 5 * i + 4] = as_dtype(res[2 + 5 * i + 4], mdt[i]);
        res[0] = gu;
        if (has_w) res[1] = at::cat(gws);
        return res;
    }
};

variable_list multi(const Tensor& u, const std::optional<Tensor>& weights, std::vector<Tensor> flat,
                    std::vector<int64_t> desc_addrs, int64_t sps, bool want_sums, int64_t ckpt_mode, std::vector<int64_t> masks,
                    double amax) {
    const Tensor w = (weights.has_value() && weights->defined()) ? *weights : Tensor();
    const std::optional<Tensor> wo = w.defined() ? std::optional<Tensor>(w) : std::nullopt;
    bool params = w.defined() && w.requires_grad();
    for (const auto& t : flat) params = params || t.requires_grad();
    return MultiFn::apply(u, wo, at::TensorList(flat), desc_addrs, sps, want_sums, ckpt_mode, masks, amax,
                          grad_mode_of(u, params));
}

// ---- the adjoint of a node that is linear in its input, differentiable once more (functional._LinearAdjointFn) -----------
// forward: the node's own backward body, unchanged (backward_now), as a function of the cotangents and of the original
// parameter tensors.  backward: for the cotangent v of gu, the node's own apply at v — through its public wrapper, with the
// original parameters, the node's descriptor(s) and its checkpoint plan — whose outputs are the cotangents' gradients, and
// torch::autograd::grad of them for the parameters'.  The parameter gradients of the first backward are handed through and
// are NOT differentiable: a cotangent on one raises (NotImplementedError in Python).  It keeps copies of what it needs of
// the outer node, which may be gone by the time it runs.
struct AdjointFn : public torch::autograd::Function<AdjointFn> {
    struct Layout {                       // where the defined results of the body sit among the node's forward arguments
        size_t n = 0;
        std::vector<size_t> pos;
    };

    // cots: the cotangents that came, cot_at: their places among the node's outputs, then the number of those outputs (a
    // shared-input group may get a cotangent on some of its outputs only, and an undefined tensor is no argument of apply)
    static variable_list forward(AutogradContext* ctx, at::TensorList cots, at::TensorList params, std::vector<int64_t> cot_at,
                                 int64_t kind, int64_t outer, int64_t layout_out, std::string descs, std::vector<int64_t> cfg,
                                 double amax) {
        ctx->set_materialize_grads(false);
        AutogradContext* node = reinterpret_cast<AutogradContext*>(outer);
        variable_list g((size_t)cot_at.back());
        for (size_t k = 0; k < cots.size(); ++k) g[(size_t)cot_at[k]] = cots[k];
        variable_list all = kind == kAdi     ? AdiFn::backward_now(node, g)
                            : kind == kSmall ? SmallFn::backward_now(node, g)
                            : kind == kMixed ? MixedFn::backward_now(node, g)
                                             : MultiFn::backward_now(node, g);
        Layout* lay = reinterpret_cast<Layout*>(layout_out);
        lay->n = all.size();
        variable_list res;
        for (size_t i = 0; i < all.size(); ++i)
            if (all[i].defined()) {
                res.push_back(all[i]);
                lay->pos.push_back(i);
            }
        variable_list save(cots.begin(), cots.end());
        save.insert(save.end(), params.begin(), params.end());
        ctx->save_for_backward(save);
        ctx->saved_data["kind"] = kind;
        ctx->saved_data["cot_at"] = cot_at;
        ctx->saved_data["n"] = std::vector<int64_t>{(int64_t)cots.size(), (int64_t)params.size()};
        ctx->saved_data["desc"] = descs;
        ctx->saved_data["cfg"] = cfg;
        ctx->saved_data["amax"] = amax;
        return res;
    }

    // the node's own apply at v: one output per cotangent of its backward
    static variable_list primal(int64_t kind, const Tensor& v, const Tensor* p, size_t np, const std::string& descs,
                                const std::vector<int64_t>& cfg, double amax);

    static variable_list backward(AutogradContext* ctx, variable_list gouts) {
        for (size_t i = 1; i < gouts.size(); ++i)
            TORCH_CHECK_NOT_IMPLEMENTED(!gouts[i].defined(),
                "the parameter gradients of a PDE layer's first backward are not differentiable: they are nonlinear in the "
                "parameters, and their derivative with respect to the input or the cotangent is a coefficient tangent the "
                "library has no kernel for (differentiate the input gradient instead, or detach them)");
        auto saved = ctx->get_saved_variables();
        auto n = ctx->saved_data["n"].toIntVector();
        const size_t n_cot = (size_t)n[0], n_par = (size_t)n[1];
        variable_list res(n_cot + n_par + 7);                 // the cotangents, the parameters, seven non-tensor arguments
        if (!gouts[0].defined()) return res;
        auto cot_at = ctx->saved_data["cot_at"].toIntVector();
        const Tensor* cots = saved.data();
        const Tensor* params = saved.data() + n_cot;
        variable_list need;
        std::vector<size_t> need_at;
        for (size_t i = 0; i < n_par; ++i)
            if (params[i].defined() && params[i].requires_grad()) {
                need.push_back(params[i]);
                need_at.push_back(i);
            }
        const bool create = at::GradMode::is_enabled();
        at::AutoGradMode mode(create || !need.empty());
        variable_list outs = primal(ctx->saved_data["kind"].toInt(), gouts[0], params, n_par, ctx->saved_data["desc"].toStringRef(),
                                    ctx->saved_data["cfg"].toIntVector(), ctx->saved_data["amax"].toDouble());
        if (!need.empty()) {
            variable_list o, c;
            for (size_t k = 0; k < n_cot; ++k)
                if (outs[(size_t)cot_at[k]].requires_grad()) {
                    o.push_back(outs[(size_t)cot_at[k]]);
                    c.push_back(cots[k]);
                }
            if (!o.empty()) {
                variable_list gp = torch::autograd::grad(o, need, c, /*retain_graph=*/create, /*create_graph=*/create,
                                                         /*allow_unused=*/true);
                for (size_t k = 0; k < need_at.size(); ++k) res[n_cot + need_at[k]] = gp[k];
            }
        }
        for (size_t k = 0; k < n_cot; ++k) res[k] = create ? outs[(size_t)cot_at[k]] : outs[(size_t)cot_at[k]].detach();
        return res;
    }
};

variable_list AdjointFn::primal(int64_t kind, const Tensor& v, const Tensor* p, size_t np, const std::string& descs,
                                const std::vector<int64_t>& cfg, double amax) {
    // cfg: {ckpt_mode, ckpt_lo, ckpt_hi, sweeps_per_step, mode | want_sums, has_weights, layers, their masks ...}; a lagged
    // call's explicit mask stays explicit, its coefficient maxima go to nobody
    const int64_t ckpt_mode = cfg[0] == 2 ? 0 : cfg[0];
    std::vector<PdeAdiDesc> d(descs.size() / sizeof(PdeAdiDesc));
    std::memcpy(d.data(), descs.data(), d.size() * sizeof(PdeAdiDesc));
    const int64_t d0 = (int64_t) reinterpret_cast<intptr_t>(d.data());
    if (kind == kAdi) return {adi(v, p[0], p[1], p[2], p[3], d0, ckpt_mode, cfg[1], cfg[2], amax)};
    if (kind == kSmall)
        return {small(v, p[0], p[1], p[2], p[3], p[4], np > 5 ? std::optional<Tensor>(p[5]) : std::nullopt, d0, cfg[3], cfg[4],
                      ckpt_mode, cfg[1], amax)};
    if (kind == kMixed) return {mixed(v, p[0], p[1], p[2], p[3], p[4], d0, cfg[3], cfg[4], ckpt_mode, cfg[1], amax)};
    const size_t nl = (size_t)cfg[6];
    std::vector<Tensor> flat(p, p + 5 * nl);
    std::vector<int64_t> addrs, masks(cfg.begin() + 7, cfg.end());
    for (size_t i = 0; i < nl; ++i) addrs.push_back((int64_t) reinterpret_cast<intptr_t>(&d[i]));
    return multi(v, cfg[5] ? std::optional<Tensor>(p[5 * nl]) : std::nullopt, flat, addrs, cfg[3], cfg[4] != 0, ckpt_mode, masks,
                 amax);
}

variable_list second_order(int64_t kind, AutogradContext* outer, const variable_list& grads) {
    auto& sd = outer->saved_data;
    std::vector<Tensor> params = sd["orig"].toTensorVector();
    std::vector<int64_t> cfg{0, 0, 0};
    if (sd.count("ckpt")) cfg = sd["ckpt"].toIntVector();
    if (kind == kSmall || kind == kMixed) {
        auto c = sd["cfg"].toIntVector();
        cfg.push_back(c[0]);
        cfg.push_back(c[1]);
    } else if (kind == kMulti) {
        auto c = sd["cfg"].toIntVector();                     // {layers, sweeps per step, plane sums, ckpt_mode, weights}
        cfg = {c[3], 0, 0, c[1], c[2], c[4], c[0]};
        std::vector<int64_t> masks = sd.count("masks") ? sd["masks"].toIntVector() : std::vector<int64_t>();
        masks.resize(c[3] == 1 ? 0 : (size_t)c[0], 0);
        cfg.insert(cfg.end(), masks.begin(), masks.end());
    }
    AdjointFn::Layout lay;
    variable_list cots;
    std::vector<int64_t> cot_at;
    for (size_t i = 0; i < grads.size(); ++i)
        if (grads[i].defined()) {
            cots.push_back(grads[i]);
            cot_at.push_back((int64_t)i);
        }
    cot_at.push_back((int64_t)grads.size());
    variable_list got = AdjointFn::apply(at::TensorList(cots), at::TensorList(params), cot_at, kind,
                                         (int64_t) reinterpret_cast<intptr_t>(outer), (int64_t) reinterpret_cast<intptr_t>(&lay),
                                         sd["desc"].toStringRef(), cfg, sd.count("amax") ? sd["amax"].toDouble() : 0.0);
    variable_list res(lay.n);
    for (size_t k = 0; k < lay.pos.size(); ++k) res[lay.pos[k]] = got[k];
    return res;
}


// ---- the Ruthotto-Haber symmetric layer (functional._SymLayerFn: cifar_2version.py:190-258) ----------------------------
// out = base + scale * (act(BatchNorm1d(X K^T)) K).  Scratch for the split strip products is kept per (device, stream,
// width): calls on one stream are ordered, and a captured graph keeps pointing at memory that stays allocated.
Tensor sym_workspace(int64_t B, int64_t D, const Tensor& like, hipStream_t st) {
    const size_t n = pde_sym_layer_workspace_bytes((int32_t)B, (int32_t)D);
    if (n == 0) return Tensor();
    // (never destroyed: device tensors must not be freed from a static destructor, after the allocator may be gone)
    static std::mutex& mu = *new std::mutex();
    static std::map<std::tuple<int, void*, int64_t, size_t>, Tensor>& cache = *new std::map<std::tuple<int, void*, int64_t, size_t>, Tensor>();
    std::lock_guard<std::mutex> g(mu);
    auto key = std::make_tuple((int)like.device().index(), (void*)st, D, n);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    if (cache.size() > 64) cache.clear();
    Tensor ws = at::empty({(int64_t)n}, like.options().dtype(at::kByte));
    cache.emplace(key, ws);
    return ws;
}

struct SymFn : public torch::autograd::Function<SymFn> {
    static Tensor forward(AutogradContext* ctx, const Tensor& X, const Tensor& K, const Tensor& gamma, const Tensor& beta,
                          const std::optional<Tensor>& base, const std::optional<Tensor>& run_mean,
                          const std::optional<Tensor>& run_var, bool training, double momentum, double eps, double scale,
                          int64_t act, bool need_grad) {
        PDE_REQUIRE(X.is_cuda() && K.is_cuda() && gamma.is_cuda() && beta.is_cuda() && (!base.has_value() || base->is_cuda()),
                    "libpdecnn_hip operators need CUDA/HIP tensors (there is no CPU fallback)");
        PDE_REQUIRE(X.dim() == 2 && K.dim() == 2 && K.size(0) == X.size(1) && K.size(1) == X.size(1), "expected X (B, D), K (D, D)");
        const int64_t B = X.size(0), D = X.size(1);
        Tensor Xf = as_f32(X), Kf = as_f32(K), gm = as_f32(gamma, false), bt = as_f32(beta, false);
        Tensor bs = base.has_value() ? as_f32(*base) : Tensor();
        c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
        hipStream_t st = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(X.device().index()).stream();
        Tensor P = at::empty({B, D}, Xf.options()), H = at::empty({B, D}, Xf.options()), out = at::empty({B, D}, Xf.options());
        Tensor mean = at::empty({D}, Xf.options()), invstd = at::empty({D}, Xf.options());
        Tensor ws = sym_workspace(B, D, Xf, st);
        float* rm = run_mean.has_value() ? run_mean->data_ptr<float>() : nullptr;
        float* rv = run_var.has_value() ? run_var->data_ptr<float>() : nullptr;
        check(pde_sym_layer_forward((int32_t)B, (int32_t)D, (int32_t)act, training ? 1 : 0, Xf.data_ptr<float>(),
                                    Kf.data_ptr<float>(), gm.data_ptr<float>(), bt.data_ptr<float>(), rm, rv, (float)momentum,
                                    (float)eps, bs.defined() ? bs.data_ptr<float>() : nullptr, (float)scale, P.data_ptr<float>(),
                                    H.data_ptr<float>(), mean.data_ptr<float>(), invstd.data_ptr<float>(), out.data_ptr<float>(),
                                    ws.defined() ? ws.data_ptr() : nullptr, ws.defined() ? (size_t)ws.numel() : 0, (void*)st),
              "pde_sym_layer_forward");
        if (need_grad) {
            ctx->save_for_backward({Xf, Kf, gm, P, H, mean, invstd});
            ctx->saved_data["cfg"] = std::vector<int64_t>{training ? 1 : 0, act, base.has_value() ? 1 : 0};
            ctx->saved_data["scale"] = scale;
        }
        return out;
    }

    static variable_list backward(AutogradContext* ctx, variable_list grads) {
        auto sv = ctx->get_saved_variables();
        const Tensor &Xf = sv[0], &Kf = sv[1], &gm = sv[2], &P = sv[3], &H = sv[4], &mean = sv[5], &invstd = sv[6];
        auto cfg = ctx->saved_data["cfg"].toIntVector();
        const double scale = ctx->saved_data["scale"].toDouble();
        const int64_t B = Xf.size(0), D = Xf.size(1);
        c10::hip::HIPGuardMasqueradingAsCUDA guard(Xf.device());
        hipStream_t st = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(Xf.device().index()).stream();
        Tensor g = grads[0];
        if (g.scalar_type() != at::kFloat) g = g.to(at::kFloat);
        g = aligned(g.contiguous());
        Tensor dP = at::empty_like(Xf), gX = at::empty_like(Xf), gK = at::empty_like(Kf);
        Tensor gg = at::empty({D}, Xf.options()), gb = at::empty({D}, Xf.options());
        Tensor ws = sym_workspace(B, D, Xf, st);
        check(pde_sym_layer_backward((int32_t)B, (int32_t)D, (int32_t)cfg[1], (int32_t)cfg[0], g.data_ptr<float>(), (float)scale,
                                     Xf.data_ptr<float>(), Kf.data_ptr<float>(), gm.data_ptr<float>(), P.data_ptr<float>(),
                                     H.data_ptr<float>(), mean.data_ptr<float>(), invstd.data_ptr<float>(), dP.data_ptr<float>(),
                                     gX.data_ptr<float>(), gK.data_ptr<float>(), gg.data_ptr<float>(), gb.data_ptr<float>(),
                                     ws.defined() ? ws.data_ptr() : nullptr, ws.defined() ? (size_t)ws.numel() : 0, (void*)st),
              "pde_sym_layer_backward");
        return once_differentiable(grads, {gX, gK, gg, gb, cfg[2] ? g : Tensor(), Tensor(), Tensor(), Tensor(), Tensor(),
                                           Tensor(), Tensor(), Tensor(), Tensor()});
    }
};

Tensor sym(const Tensor& X, const Tensor& K, const Tensor& gamma, const Tensor& beta, const std::optional<Tensor>& base,
           const std::optional<Tensor>& run_mean, const std::optional<Tensor>& run_var, bool training, double momentum, double eps,
           double scale, int64_t act) {
    const bool need_grad = at::GradMode::is_enabled() && (X.requires_grad() || K.requires_grad() || gamma.requires_grad() ||
                                                          beta.requires_grad() || (base.has_value() && base->requires_grad()));
    auto opt = [](const std::optional<Tensor>& t) { return (t.has_value() && t->defined()) ? t : std::optional<Tensor>(); };
    return SymFn::apply(X, K, gamma, beta, opt(base), opt(run_mean), opt(run_var), training, momentum, eps, scale, act, need_grad);
}

// ---- the same layer under fp16 / bf16 autocast (functional._SymLayerF16Fn, _SymLayerBf16Fn): 16-bit operands, K16 = r(K)
// precomputed by the caller.  out is a 16-bit tensor without a base (F_sym), fp32 with one.  Scratch comes from the caching
// allocator for every call: nothing is kept between calls (a captured graph owns what its capture allocated).
// One implementation over the element's dtype and entry points; the two nodes differ in those alone.
struct F16Api {
    static constexpr at::ScalarType dtype = at::kHalf;
    static constexpr auto k_to = &pde_sym_k_to_f16;
    static constexpr auto workspace_bytes = &pde_sym_layer_f16_workspace_bytes;
    static constexpr auto forward = &pde_sym_layer_f16_forward;
    static constexpr auto backward = &pde_sym_layer_f16_backward;
    static constexpr const char* k_to_name = "pde_sym_k_to_f16";
    static constexpr const char* forward_name = "pde_sym_layer_f16_forward";
    static constexpr const char* backward_name = "pde_sym_layer_f16_backward";
    static constexpr const char* k16_msg = "expected X (B, D) and a contiguous fp16 K16 (D, D)";
};
struct Bf16Api {
    static constexpr at::ScalarType dtype = at::kBFloat16;
    static constexpr auto k_to = &pde_sym_k_to_bf16;
    static constexpr auto workspace_bytes = &pde_sym_layer_bf16_workspace_bytes;
    static constexpr auto forward = &pde_sym_layer_bf16_forward;
    static constexpr auto backward = &pde_sym_layer_bf16_backward;
    static constexpr const char* k_to_name = "pde_sym_k_to_bf16";
    static constexpr const char* forward_name = "pde_sym_layer_bf16_forward";
    static constexpr const char* backward_name = "pde_sym_layer_bf16_backward";
    static constexpr const char* k16_msg = "expected X (B, D) and a contiguous bf16 K16 (D, D)";
};

template <class Api>
Tensor sym_k16_as(const Tensor& K) {
    PDE_REQUIRE(K.is_cuda() && K.dim() == 2 && K.size(0) == K.size(1), "expected a square CUDA K");
    Tensor Kf = as_f32(K.detach());
    c10::hip::HIPGuardMasqueradingAsCUDA guard(K.device());
    hipStream_t st = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(K.device().index()).stream();
    Tensor K16 = at::empty(K.sizes(), Kf.options().dtype(Api::dtype));
    check(Api::k_to((int32_t)K.size(0), Kf.data_ptr<float>(), reinterpret_cast<uint16_t*>(K16.data_ptr()), (void*)st),
          Api::k_to_name);
    return K16;
}
Tensor sym_k16(const Tensor& K) { return sym_k16_as<F16Api>(K); }
Tensor sym_kbf16(const Tensor& K) { return sym_k16_as<Bf16Api>(K); }

template <class Api>
Tensor sym16_workspace(int64_t B, int64_t D, const Tensor& like) {
    const size_t n = Api::workspace_bytes((int32_t)B, (int32_t)D);
    return at::empty({(int64_t)n}, like.options().dtype(at::kByte));
}

uint16_t* h16(const Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

template <class Fn, class Api>
struct Sym16Node : public torch::autograd::Function<Fn> {
    static Tensor forward(AutogradContext* ctx, const Tensor& X, const Tensor& K, const Tensor& K16, const Tensor& gamma,
                          const Tensor& beta, const std::optional<Tensor>& base, const std::optional<Tensor>& run_mean,
                          const std::optional<Tensor>& run_var, bool training, double momentum, double eps, double scale,
                          int64_t act, bool need_grad) {
        PDE_REQUIRE(X.is_cuda() && K16.is_cuda() && gamma.is_cuda() && beta.is_cuda() && (!base.has_value() || base->is_cuda()),
                    "libpdecnn_hip operators need CUDA/HIP tensors (there is no CPU fallback)");
        PDE_REQUIRE(X.dim() == 2 && K16.dim() == 2 && K16.size(0) == X.size(1) && K16.size(1) == X.size(1) &&
                    K16.scalar_type() == Api::dtype && K16.is_contiguous(), Api::k16_msg);
        const int64_t B = X.size(0), D = X.size(1);
        Tensor Xf = as_f32(X), gm = as_f32(gamma, false), bt = as_f32(beta, false);
        Tensor bs = base.has_value() ? as_f32(*base) : Tensor();
        const Tensor K16a = aligned(K16);
        c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
        hipStream_t st = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(X.device().index()).stream();
        const auto h = Xf.options().dtype(Api::dtype);
        Tensor P = at::empty({B, D}, h), H = at::empty({B, D}, h);
        Tensor out = bs.defined() ? at::empty({B, D}, Xf.options()) : at::empty({B, D}, h);
        Tensor mean = at::empty({D}, Xf.options()), invstd = at::empty({D}, Xf.options());
        Tensor ws = sym16_workspace<Api>(B, D, Xf);
        float* rm = run_mean.has_value() ? run_mean->data_ptr<float>() : nullptr;
        float* rv = run_var.has_value() ? run_var->data_ptr<float>() : nullptr;
        check(Api::forward((int32_t)B, (int32_t)D, (int32_t)act, training ? 1 : 0, Xf.data_ptr<float>(), h16(K16a),
                           gm.data_ptr<float>(), bt.data_ptr<float>(), rm, rv, (float)momentum, (float)eps,
                           bs.defined() ? bs.data_ptr<float>() : nullptr, (float)scale, h16(P), h16(H),
                           mean.data_ptr<float>(), invstd.data_ptr<float>(), out.data_ptr(), ws.data_ptr(),
                           (size_t)ws.numel(), (void*)st),
              Api::forward_name);
        if (need_grad) {
            ctx->save_for_backward({Xf, K16a, gm, P, H, mean, invstd});
            ctx->saved_data["cfg"] = std::vector<int64_t>{training ? 1 : 0, act, base.has_value() ? 1 : 0};
            ctx->saved_data["scale"] = scale;
        }
        return out;
    }

    static variable_list backward(AutogradContext* ctx, variable_list grads) {
        auto sv = ctx->get_saved_variables();
        const Tensor &Xf = sv[0], &K16 = sv[1], &gm = sv[2], &P = sv[3], &H = sv[4], &mean = sv[5], &invstd = sv[6];
        auto cfg = ctx->saved_data["cfg"].toIntVector();
        const double scale = ctx->saved_data["scale"].toDouble();
        const int64_t B = Xf.size(0), D = Xf.size(1);
        c10::hip::HIPGuardMasqueradingAsCUDA guard(Xf.device());
        hipStream_t st = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(Xf.device().index()).stream();
        Tensor g = grads[0];
        if (g.scalar_type() != at::kFloat) g = g.to(at::kFloat);
        g = aligned(g.contiguous());
        Tensor dP = at::empty({B, D}, P.options()), gX = at::empty_like(Xf), gK = at::empty({D, D}, Xf.options());
        Tensor gg = at::empty({D}, Xf.options()), gb = at::empty({D}, Xf.options());
        Tensor ws = sym16_workspace<Api>(B, D, Xf);
        check(Api::backward((int32_t)B, (int32_t)D, (int32_t)cfg[1], (int32_t)cfg[0], g.data_ptr<float>(), (float)scale,
                            Xf.data_ptr<float>(), h16(K16), gm.data_ptr<float>(), h16(P), h16(H),
                            mean.data_ptr<float>(), invstd.data_ptr<float>(), h16(dP), gX.data_ptr<float>(),
                            gK.data_ptr<float>(), gg.data_ptr<float>(), gb.data_ptr<float>(), ws.data_ptr(),
                            (size_t)ws.numel(), (void*)st),
              Api::backward_name);
        return once_differentiable(grads, {gX, gK, Tensor(), gg, gb, cfg[2] ? g : Tensor(), Tensor(), Tensor(), Tensor(),
                                           Tensor(), Tensor(), Tensor(), Tensor(), Tensor()});
    }
};
struct SymF16Fn : public Sym16Node<SymF16Fn, F16Api> {};
struct SymBf16Fn : public Sym16Node<SymBf16Fn, Bf16Api> {};

template <class Fn>
Tensor sym16(const Tensor& X, const Tensor& K, const Tensor& K16, const Tensor& gamma, const Tensor& beta,
             const std::optional<Tensor>& base, const std::optional<Tensor>& run_mean, const std::optional<Tensor>& run_var,
             bool training, double momentum, double eps, double scale, int64_t act) {
    const bool need_grad = at::GradMode::is_enabled() && (X.requires_grad() || K.requires_grad() || gamma.requires_grad() ||
                                                          beta.requires_grad() || (base.has_value() && base->requires_grad()));
    auto opt = [](const std::optional<Tensor>& t) { return (t.has_value() && t->defined()) ? t : std::optional<Tensor>(); };
    return Fn::apply(X, K, K16, gamma, beta, opt(base), opt(run_mean), opt(run_var), training, momentum, eps, scale, act,
                     need_grad);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "native host path of the launch-bound PDE-layer calls (torch C++ autograd over the C ABI of pdecnn.h)";
    m.def("adi", &adi, "functional.adi_diffuse without the interpreter: one implicit diffusion layer call",
          py::arg("u"), py::arg("alpha_base"), py::arg("beta_base"), py::arg("alpha_time_coeff"), py::arg("beta_time_coeff"),
          py::arg("desc_addr"), py::arg("ckpt_mode"), py::arg("ckpt_lo"), py::arg("ckpt_hi"), py::arg("amax"));
    py::class_<Ticket, std::shared_ptr<Ticket>>(m, "Ticket", "the per-sweep coefficient maxima of one call (pinned slot + event)")
        .def("query", &Ticket::query)
        .def("synchronize", &Ticket::synchronize)
        .def("wait", [](std::shared_ptr<Ticket> t) {
            t->synchronize();
            std::vector<float> v(t->slot->host, t->slot->host + t->n);
            return v;
        })
        .def_property_readonly("host", &Ticket::host)
        .def_property_readonly("event", [](std::shared_ptr<Ticket> t) { return t; });
    m.def("adi_lagged", &adi_lagged, "adi with an explicit checkpoint mask that also delivers this call's coefficient maxima",
          py::arg("u"), py::arg("alpha_base"), py::arg("beta_base"), py::arg("alpha_time_coeff"), py::arg("beta_time_coeff"),
          py::arg("desc_addr"), py::arg("ckpt_lo"), py::arg("ckpt_hi"));
    m.def("small", &small, "functional.adi_diffuse_small: one layer with a channel operator, C <= 4, one launch per pass",
          py::arg("u"), py::arg("alpha_base"), py::arg("beta_base"), py::arg("alpha_time_coeff"), py::arg("beta_time_coeff"),
          py::arg("M"), py::arg("skip_weight"), py::arg("desc_addr"), py::arg("sweeps_per_step"), py::arg("mode"),
          py::arg("ckpt_mode"), py::arg("ckpt_lo"), py::arg("amax"));
    m.def("mixed", &mixed, "functional.adi_diffuse_mixed: one layer with a channel operator between its steps, any width",
          py::arg("u"), py::arg("alpha_base"), py::arg("beta_base"), py::arg("alpha_time_coeff"), py::arg("beta_time_coeff"),
          py::arg("M"), py::arg("desc_addr"), py::arg("sweeps_per_step"), py::arg("mode"), py::arg("ckpt_mode"),
          py::arg("ckpt_lo"), py::arg("amax"));
    m.def("multi", &multi, "functional.adi_diffuse_multi: layers that share an input, one launch per pass",
          py::arg("u"), py::arg("weights"), py::arg("flat"), py::arg("desc_addrs"), py::arg("sweeps_per_step"),
          py::arg("want_sums"), py::arg("ckpt_mode"), py::arg("masks"), py::arg("amax"));
    m.def("sym", &sym, "functional.sym_layer's autograd node: out = base + scale * (act(BatchNorm1d(X K^T)) K)",
          py::arg("X"), py::arg("K"), py::arg("gamma"), py::arg("beta"), py::arg("base"), py::arg("running_mean"),
          py::arg("running_var"), py::arg("training"), py::arg("momentum"), py::arg("eps"), py::arg("scale"), py::arg("act"));
    m.def("sym_k16", &sym_k16, "K16 = r(K): the fp16 copy of a symmetric layer's weight (one per autocast block forward)",
          py::arg("K"));
    m.def("sym_f16", &sym16<SymF16Fn>, "functional.sym_layer's fp16-operand autograd node (fp16 autocast's rounding points)",
          py::arg("X"), py::arg("K"), py::arg("K16"), py::arg("gamma"), py::arg("beta"), py::arg("base"), py::arg("running_mean"),
          py::arg("running_var"), py::arg("training"), py::arg("momentum"), py::arg("eps"), py::arg("scale"), py::arg("act"));
    m.def("sym_kbf16", &sym_kbf16, "K16 = r(K): the bf16 copy of a symmetric layer's weight (one per autocast block forward)",
          py::arg("K"));
    m.def("sym_bf16", &sym16<SymBf16Fn>, "functional.sym_layer's bf16-operand autograd node (bf16 autocast's rounding points)",
          py::arg("X"), py::arg("K"), py::arg("K16"), py::arg("gamma"), py::arg("beta"), py::arg("base"), py::arg("running_mean"),
          py::arg("running_var"), py::arg("training"), py::arg("momentum"), py::arg("eps"), py::arg("scale"), py::arg("act"));
    m.def("set_error_class", [](py::object cls) {
        Py_XDECREF(g_error_class);
        g_error_class = cls.release().ptr();
    }, "the Python exception class failed calls of the C ABI raise (_lib.PdeError)");
    py::register_exception_translator([](std::exception_ptr p) {
        try {
            if (p) std::rethrow_exception(p);
        } catch (const PdeFailure& e) {
            PyErr_SetString(g_error_class ? g_error_class : PyExc_RuntimeError, e.what());
        }
    });
    m.def("abi_version", []() { return std::string(pde_version()); });
}
