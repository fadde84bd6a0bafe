#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>

namespace rd {

// =================================================================================================
// safetensors image -> WeightStore.  Format: u64 LE header length, JSON header
// {"name": {"dtype": "F32", "shape": [...], "data_offsets": [b, e]}, "__metadata__": {...}}, raw data.
// (what the reference loads with safetensors.torch.load_file, rapid_doc/model/ocr/torch.py:93-110)
// =================================================================================================
namespace {
struct JsonCur {
    const char* p;
    const char* end;
    void ws() {
        while (p < end && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) ++p;
    }
    bool eat(char c) {
        ws();
        if (p < end && *p == c) { ++p; return true; }
        return false;
    }
    void expect(char c) {
        if (!eat(c)) throw Error(std::string("safetensors header: expected '") + c + "'");
    }
    std::string str() {
        ws();
        if (p >= end || *p != '"') throw Error("safetensors header: expected string");
        ++p;
        std::string out;
        while (p < end && *p != '"') {
            if (*p == '\\' && p + 1 < end) {
                ++p;
                switch (*p) {
                    case 'n': out += '\n'; break;
                    case 't': out += '\t'; break;
                    case 'u': out += '?'; p += 4; break;
                    default: out += *p;
                }
                ++p;
            } else {
                out += *p++;
            }
        }
        if (p >= end) throw Error("safetensors header: unterminated string");
        ++p;
        return out;
    }
    int64_t integer() {
        ws();
        bool neg = false;
        if (p < end && *p == '-') { neg = true; ++p; }
        if (p >= end || *p < '0' || *p > '9') throw Error("safetensors header: expected integer");
        int64_t v = 0;
        while (p < end && *p >= '0' && *p <= '9') v = v * 10 + (*p++ - '0');
        return neg ? -v : v;
    }
    void skip_value() {
        ws();
        if (p >= end) throw Error("safetensors header: truncated");
        if (*p == '"') { str(); return; }
        if (*p == '{') {
            ++p;
            if (eat('}')) return;
            do { str(); expect(':'); skip_value(); } while (eat(','));
            expect('}');
            return;
        }
        if (*p == '[') {
            ++p;
            if (eat(']')) return;
            do { skip_value(); } while (eat(','));
            expect(']');
            return;
        }
        while (p < end && *p != ',' && *p != '}' && *p != ']') ++p;
    }
};
size_t dtype_size(const std::string& d) {
    if (d == "F32" || d == "I32" || d == "U32") return 4;
    if (d == "F64" || d == "I64" || d == "U64") return 8;
    if (d == "F16" || d == "BF16" || d == "I16" || d == "U16") return 2;
    if (d == "U8" || d == "I8" || d == "BOOL") return 1;
    throw Error("safetensors: unsupported dtype " + d);
}
}  // namespace

void WeightStore::load_safetensors(const void* blob, size_t nbytes) {
    RD_CHECK(blob && nbytes >= 8, "weights: empty image");
    uint64_t hlen = 0;
    std::memcpy(&hlen, blob, 8);
    RD_CHECK(hlen > 0 && 8 + hlen <= nbytes, "weights: bad safetensors header length");
    blob_.assign((const uint8_t*)blob, (const uint8_t*)blob + nbytes);
    map_.clear();
    const uint8_t* base = blob_.data() + 8 + hlen;
    const size_t data_bytes = nbytes - 8 - hlen;
    JsonCur c{(const char*)blob_.data() + 8, (const char*)blob_.data() + 8 + hlen};
    c.expect('{');
    if (!c.eat('}')) {
        do {
            std::string name = c.str();
            c.expect(':');
            if (name == "__metadata__") { c.skip_value(); continue; }
            HostTensor t;
            int64_t b = -1, e = -1;
            c.expect('{');
            do {
                std::string k = c.str();
                c.expect(':');
                if (k == "dtype") t.dtype = c.str();
                else if (k == "shape") {
                    c.expect('[');
                    if (!c.eat(']')) {
                        do { t.shape.push_back(c.integer()); } while (c.eat(','));
                        c.expect(']');
                    }
                } else if (k == "data_offsets") {
                    c.expect('[');
                    b = c.integer();
                    c.expect(',');
                    e = c.integer();
                    c.expect(']');
                } else c.skip_value();
            } while (c.eat(','));
            c.expect('}');
            RD_CHECK(b >= 0 && e >= b && (size_t)e <= data_bytes, "weights: tensor offsets out of range: " + name);
            RD_CHECK((size_t)(e - b) == t.numel() * dtype_size(t.dtype), "weights: tensor byte size mismatch: " + name);
            t.data = base + b;
            t.nbytes = (size_t)(e - b);
            if (name.rfind("model.", 0) == 0) name = name.substr(6);  // reference torch.py:105-110
            map_[name] = std::move(t);
        } while (c.eat(','));
        c.expect('}');
    }
    RD_CHECK(!map_.empty(), "weights: no tensors in image");
}

void WeightStore::add_derived(const std::string& name, const std::vector<int64_t>& shape, std::vector<float>&& data) {
    derived_.push_back(std::make_unique<std::vector<float>>(std::move(data)));
    HostTensor t;
    t.shape = shape;
    t.dtype = "F32";
    t.data = reinterpret_cast<const uint8_t*>(derived_.back()->data());
    t.nbytes = derived_.back()->size() * sizeof(float);
    RD_CHECK(t.numel() * sizeof(float) == t.nbytes, "derived tensor size mismatch: " + name);
    map_[name] = std::move(t);
}

const HostTensor& WeightStore::get(const std::string& name) const {
    auto it = map_.find(name);
    if (it == map_.end()) throw Error("weights: missing tensor '" + name + "'");
    if (it->second.dtype != "F32") throw Error("weights: tensor '" + name + "' is " + it->second.dtype + ", expected F32");
    return it->second;
}

// =================================================================================================
ParamBlock::~ParamBlock() {
    if (dev_) (void)hipFree(dev_);
}
size_t ParamBlock::add(const std::string& key, const std::vector<float>& v) {
    RD_CHECK(!dev_, "ParamBlock: add after upload");
    auto it = off_.find(key);
    if (it != off_.end()) return it->second;
    size_t off = (host_.size() + 63) & ~size_t(63);  // 256-byte aligned
    host_.resize(off + v.size(), 0.f);
    std::copy(v.begin(), v.end(), host_.begin() + off);
    off_[key] = off;
    return off;
}
size_t ParamBlock::add_u16(const std::string& key, const std::vector<uint16_t>& v) {
    std::vector<float> packed((v.size() + 1) / 2, 0.f);
    std::memcpy(packed.data(), v.data(), v.size() * sizeof(uint16_t));
    return add(key, packed);
}
void ParamBlock::upload() {
    if (dev_) { (void)hipFree(dev_); dev_ = nullptr; }
    size_t n = std::max<size_t>(host_.size(), 64) + 64;
    RD_HIP(hipMalloc((void**)&dev_, n * sizeof(float)));
    RD_HIP(hipMemcpy(dev_, host_.data(), host_.size() * sizeof(float), hipMemcpyHostToDevice));
}
const float* ParamBlock::ptr(const std::string& key) const {
    auto it = off_.find(key);
    if (it == off_.end()) throw Error("params: missing folded tensor '" + key + "'");
    RD_CHECK(dev_, "params: not uploaded");
    return dev_ + it->second;
}

const float* ParamBlock::host_ptr(const std::string& key) const {
    auto it = off_.find(key);
    if (it == off_.end()) throw Error("params: missing folded tensor '" + key + "'");
    return host_.data() + it->second;
}

Plan::~Plan() {
    // a plan is dropped only by the LRU of Engine::plan_for (rare): wait for the stream an exec was last launched on before
    // freeing it - its kernel arguments live in the exec
    for (auto& g : graphs)
        if (g.exec) {
            (void)hipStreamSynchronize(g.stream);
            (void)hipGraphExecDestroy(g.exec);
        }
    (void)hipGetLastError();
}

// =================================================================================================
// Engine
// =================================================================================================
extern bool g_disable_fused_mixer;
Engine::Engine(int device, const std::string& kind) : device_(device), kind_(kind), model_(find_model(kind)) {
    if (const char* e = getenv("RD_DISABLE_FUSED_MIXER")) g_disable_fused_mixer = e[0] == '1';   // (a process-wide flag: unset leaves it as it is)
    if (rd_env_off("RD_GRAPHS")) graphs_ = false;
    if (const char* e = getenv("RD_PRECISION")) {
        const std::string v(e);
        RD_CHECK(v == "auto" || v == "fp32" || v == "h3", "RD_PRECISION must be auto, fp32 or h3");
        precision_ = v == "h3" ? PREC_H3 : v == "fp32" ? PREC_FP32 : PREC_AUTO;
    }
    RD_CHECK(model_ != nullptr, "unknown model kind '" + kind + "'");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) throw Error("no HIP device available (MI355X required; there is no CPU fallback)");
    RD_CHECK(device >= 0 && device < count, "device id out of range");
}

void Engine::retire_graph(hipGraphExec_t exec, hipStream_t s) {
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess && hipEventRecord(ev, s) == hipSuccess) {
        retired_graphs_.push_back({exec, ev});
        return;
    }
    if (ev) (void)hipEventDestroy(ev);
    (void)hipGetLastError();
    (void)hipStreamSynchronize(s);            // no event: wait, then free
    (void)hipGraphExecDestroy(exec);
}

void Engine::sweep_retired_graphs(bool wait) {
    size_t keep = 0;
    for (auto& r : retired_graphs_) {
        if (wait) (void)hipEventSynchronize(r.done);
        if (wait || hipEventQuery(r.done) == hipSuccess) {
            (void)hipGraphExecDestroy(r.exec);
            (void)hipEventDestroy(r.done);
        } else {
            retired_graphs_[keep++] = r;
        }
    }
    retired_graphs_.resize(keep);
    (void)hipGetLastError();                  // hipErrorNotReady of the queries
}

Engine::~Engine() {
    (void)hipSetDevice(device_);
    sweep_retired_graphs(true);
    for (auto ev : events_) (void)hipEventDestroy(ev);
    if (arena_) (void)hipFree(arena_);
    if (range_flag_host_) (void)hipHostFree(range_flag_host_);
}

void Engine::load_weights(const void* blob, size_t nbytes) {
    RD_HIP(hipSetDevice(device_));
    RD_CHECK(!loaded_, "weights already loaded for this handle");
    store_.load_safetensors(blob, nbytes);
    if (model_->n_classes_tensor) {
        n_classes_ = (int)store_.get(model_->n_classes_tensor).shape[0];
        rec_token_dim_ = (int)store_.get(model_->token_dim_tensor).shape[1];
    }
    if (model_->derive) model_->derive(store_);
    if (kind_ == "ppocrv5_det_server" || kind_ == "ppocrv5_rec_server") backbone_ = store_.has(pphgnet_small_marker()) ? "pphgnet_small" : "pphgnetv2_b4";
    Plan dummy;
    h3_prepared_ = precision_ == PREC_H3;
    // the range flag: one word of pinned host memory mapped into the device's address space (rd_device.h rd_raise_flag) - reading
    // it costs a stream synchronise and a host load, not a device-to-host copy that queues behind whatever shares its hardware queue
    RD_HIP(hipHostMalloc((void**)&range_flag_host_, 64, hipHostMallocMapped | hipHostMallocCoherent));
    *range_flag_host_ = 0u;
    RD_HIP(hipHostGetDevicePointer((void**)&range_flag_, (void*)range_flag_host_, 0));
    Builder b(Mode::PREPARE, &store_, &params_, &dummy, h3_prepared_, true);
    for (const ModelDesc::Geom& g : model_->prepare) model_->build(b, g.B, g.H, g.W, g.flags);
    params_.upload();
    loaded_ = true;
}

void Engine::set_precision(int p) {
    RD_CHECK(p == PREC_AUTO || p == PREC_FP32 || p == PREC_H3, "unknown precision mode");
    RD_CHECK(p != PREC_H3 || h3_prepared_ || !loaded_, "precision h3 needs RD_PRECISION=h3 when the weights are loaded");
    precision_ = p;
}

int Engine::take_range_flag(hipStream_t s) {
    if (!range_flag_host_) return 0;
    RD_HIP(hipSetDevice(device_));
    RD_HIP(hipStreamSynchronize(s));            // the forwards to be judged were launched on s, or s waits on their events
    const unsigned v = __atomic_load_n(range_flag_host_, __ATOMIC_ACQUIRE);
    if (v) __atomic_store_n(range_flag_host_, 0u, __ATOMIC_RELEASE);
    return v ? 1 : 0;
}

const Plan& Engine::plan_for(int B, int H, int W, int flags) {
    RD_CHECK(loaded_, "weights not loaded");
    auto key = std::make_tuple(B, H, W, flags | (precision_ << 24));
    auto it = plans_.find(key);
    if (it != plans_.end()) {
        it->second->last_use = ++plan_clock_;
        return *it->second;
    }
    // LRU: one cold shape (a long line, an odd page size) must not throw away the hot plans of this handle
    while (plans_.size() >= kMaxPlans) {
        auto victim = plans_.begin();
        for (auto j = plans_.begin(); j != plans_.end(); ++j)
            if (j->second->last_use < victim->second->last_use) victim = j;
        plans_.erase(victim);
    }
    ++plans_built_;
    auto plan = std::make_unique<Plan>();
    Builder b(Mode::PLAN, &store_, &params_, plan.get(), precision_ == PREC_H3, precision_ == PREC_AUTO, range_flag_);
    model_->build(b, B, H, W, flags);
    plan->arena_bytes = (plan->arena_bytes + 255) / 256 * 256;
    plan->last_use = ++plan_clock_;
    auto& ref = *plan;
    plans_[key] = std::move(plan);
    return ref;
}

void Engine::run(int B, int H, int W, int flags, const std::vector<void*>& ext, void* ws, size_t ws_bytes, hipStream_t s) {
    RD_HIP(hipSetDevice(device_));
    const Plan& plan = plan_for(B, H, W, flags);
    RunCtx ctx;
    ctx.ext = ext;
    ctx.stream = s;
    if (ws) {
        RD_CHECK(ws_bytes >= plan.arena_bytes, "workspace too small");
        ctx.arena = (uint8_t*)ws;
    } else {
        if (arena_bytes_ < plan.arena_bytes) {
            RD_HIP(hipStreamSynchronize(s));
            if (arena_) RD_HIP(hipFree(arena_));
            arena_ = nullptr;
            arena_bytes_ = 0;
            RD_HIP(hipMalloc((void**)&arena_, plan.arena_bytes));
            arena_bytes_ = plan.arena_bytes;
            // developer check (RD_POISON_ARENA=1): fresh workspace filled with NaN bit patterns - no kernel may let workspace bytes
            // it did not write reach a result or the range guard
            static const bool poison = rd_env_on("RD_POISON_ARENA");
            if (poison) {     // on the launch stream: a null-stream memset is not ordered against a non-blocking stream
                RD_HIP(hipMemsetAsync(arena_, 0xFF, arena_bytes_, s));
                RD_HIP(hipStreamSynchronize(s));
            }
        }
        ctx.arena = arena_;
    }
    for (const Buf& b : plan.bufs)
        if (b.external >= 0) RD_CHECK(b.external < (int)ext.size() && ext[b.external], "missing external buffer");
    if (!profiling_) {
        // developer trace (RD_RANGE_TRACE=1): which op raises the split-fp16 range flag (synchronises after every op)
        static const bool range_trace = rd_env_on("RD_RANGE_TRACE");
        if (range_trace && range_flag_) {
            for (const OpRecord& op : plan.ops) {
                op.run(plan, ctx);
                RD_HIP(hipStreamSynchronize(s));
                unsigned v = __atomic_load_n(range_flag_host_, __ATOMIC_ACQUIRE);
                if (v) {
                    fprintf(stderr, "[range] %s: op '%s' kind %s cfg %s shape %s raised the flag (B=%d H=%d W=%d flags=%d)\n", kind_.c_str(),
                            op.name.c_str(), op.kind.c_str(), op.cfg.c_str(), op.shape.c_str(), B, H, W, flags);
                    break;                       // (the flag stays raised for the caller)
                }
            }
            return;
        }
        // developer what-if (timing only, results are garbage): RD_SKIP_KIND=<op kind> leaves those launches out
        static const char* skip_kind = std::getenv("RD_SKIP_KIND");
        if (skip_kind) {
            for (const OpRecord& op : plan.ops)
                if (op.kind != skip_kind) op.run(plan, ctx);
            RD_HIP(hipGetLastError());
            return;
        }
        // hipGraph replay.  A forward is 30-90 dependent launches whose arguments are fixed by (plan, external pointers, workspace):
        // the second time the same triple shows up on a stream the launches are captured into a graph, from the third on the
        // host issues ONE hipGraphLaunch (a page batch is ~900 launches: 6-10 ms of a single host thread per 95-ms step, and a
        // slow host thread was measured to cost 10 % of the throughput).  Callers keep their buffers stable (PagePipeline).
        if (graphs_ && !plan.graph_broken && plan.ops.size() >= 4) {
            GraphSlot* slot = nullptr;
            for (auto& g : plan.graphs)
                if (g.arena == ctx.arena && g.stream == s && g.ext == ext) { slot = &g; break; }
            if (slot && slot->exec) {
                slot->last_use = ++plan_clock_;
                plan.graph_evictions = 0;     // replays do happen for this plan
                ++graph_replays_;
                RD_HIP(hipGraphLaunch(slot->exec, s));
                return;
            }
            if (slot) {                       // seen once before: worth a capture
                hipGraph_t graph = nullptr;
                bool ok = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess;
                if (ok) {
                    for (const OpRecord& op : plan.ops) op.run(plan, ctx);
                    ok = hipStreamEndCapture(s, &graph) == hipSuccess && graph != nullptr;
                }
                hipGraphExec_t exec = nullptr;
                if (ok) ok = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
                if (graph) (void)hipGraphDestroy(graph);
                if (ok) {
                    ++graph_captures_;
                    slot->exec = exec;
                    slot->last_use = ++plan_clock_;
                    RD_HIP(hipGraphLaunch(exec, s));
                    return;
                }
                (void)hipGetLastError();
                plan.graph_broken = true;     // this plan does not capture: direct launches from now on
            } else {
                if (!retired_graphs_.empty()) sweep_retired_graphs(false);
                if (plan.graphs.size() >= kMaxGraphSlots) {
                    auto victim = plan.graphs.begin();
                    for (auto j = plan.graphs.begin(); j != plan.graphs.end(); ++j)
                        if (j->last_use < victim->last_use) victim = j;
                    if (victim->exec) retire_graph(victim->exec, victim->stream);   // possibly still in flight: freed after its event
                    plan.graphs.erase(victim);
                    if (++plan.graph_evictions > kMaxGraphEvictions) {
                        // the callers' pointers do not repeat for this plan (more live pointer sets than slots): every slot is
                        // evicted before it is seen again, so capturing only costs - launch directly from now on
                        for (auto& g : plan.graphs)
                            if (g.exec) retire_graph(g.exec, g.stream);
                        plan.graphs.clear();
                        plan.graph_broken = true;
                    }
                }
                if (plan.graph_broken) {
                    for (const OpRecord& op : plan.ops) op.run(plan, ctx);
                    RD_HIP(hipGetLastError());
                    return;
                }
                GraphSlot g;
                g.ext = ext; g.arena = ctx.arena; g.stream = s; g.last_use = ++plan_clock_;
                plan.graphs.push_back(std::move(g));
            }
        }
        for (const OpRecord& op : plan.ops) op.run(plan, ctx);
        RD_HIP(hipGetLastError());
        return;
    }
    const size_t need = plan.ops.size() + 1;
    while (events_.size() < need) {
        hipEvent_t ev;
        RD_HIP(hipEventCreate(&ev));
        events_.push_back(ev);
    }
    RD_HIP(hipEventRecord(events_[0], s));
    for (size_t i = 0; i < plan.ops.size(); ++i) {
        plan.ops[i].run(plan, ctx);
        RD_HIP(hipEventRecord(events_[i + 1], s));
    }
    RD_HIP(hipEventSynchronize(events_[plan.ops.size()]));
    RD_HIP(hipGetLastError());
    profile_.clear();
    for (size_t i = 0; i < plan.ops.size(); ++i) {
        float ms = 0.f;
        RD_HIP(hipEventElapsedTime(&ms, events_[i], events_[i + 1]));
        const OpRecord& op = plan.ops[i];
        profile_.push_back({op.name, op.kind, op.cfg, op.shape, op.flops, op.bytes, ms});
    }
}

std::string Engine::profile_json() const {
    std::ostringstream os;
    os << "[";
    for (size_t i = 0; i < profile_.size(); ++i) {
        const ProfileEntry& e = profile_[i];
        if (i) os << ",";
        os << "{\"name\":\"" << e.name << "\",\"kind\":\"" << e.kind << "\",\"cfg\":\"" << e.cfg << "\",\"shape\":\"" << e.shape
           << "\",\"flops\":" << e.flops
           << ",\"bytes\":" << e.bytes << ",\"ms\":" << e.ms << "}";
    }
    os << "]";
    return os.str();
}

}  // namespace rd
