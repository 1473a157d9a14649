// mg_rtc.hip — the observation kernel specialised on demand (include/marlgrid_hip.h: mg_render_specialize).  render_pick_ideal
// (mg_render_pick.h) says which instantiation of mg::render_kernel a configuration off the table would get; this file compiles
// it with hipRTC from the library's own headers — the files next to it, read once and only accepted when they are the ones it was
// built from, handed to hiprtcCreateProgram as in-memory headers —, keeps the code object (per process; per cache_dir),
// loads it on the current device and launches it with exactly what launch_render_t passes (render_launch_plan).
// libhiprtc is opened at the first call: the library loads and does everything else without it.
#include <dlfcn.h>
#include <errno.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "mg_render_kernel.h"

#ifndef MG_BUILD_ID
#define MG_BUILD_ID "unknown"
#endif

namespace {

// ---- the sources: the headers next to the library, if they are the ones it was built from ---------------------------------------
// MG_RTC_HDRS (the Makefile's $(HDRS): paths relative to the library's directory, in the order the build id hashes them) and
// MG_RTC_HDR_CKSUM (POSIX cksum of their concatenation).  The library does not carry their text: what a scan of the binary
// finds is what the binary is compiled with.
struct RtcSource { std::string name, text; };

uint32_t posix_cksum(const std::string& s) {      // CRC-32 / POSIX: polynomial 0x04C11DB7, the length appended, complemented
    uint32_t crc = 0;
    auto feed = [&crc](unsigned char c) {
        crc ^= (uint32_t)c << 24;
        for (int k = 0; k < 8; k++) crc = (crc & 0x80000000u) ? (crc << 1) ^ 0x04C11DB7u : crc << 1;
    };
    for (unsigned char c : s) feed(c);
    for (size_t n = s.size(); n; n >>= 8) feed((unsigned char)(n & 0xFF));
    return ~crc;
}

const std::vector<RtcSource>* rtc_sources(std::string* why) {
    static std::once_flag once;
    static std::vector<RtcSource> sources;
    static std::string reason;
    std::call_once(once, [] {
        Dl_info self;
        if (!dladdr((const void*)&posix_cksum, &self) || !self.dli_fname) { reason = "the library cannot tell where it was loaded from"; return; }
        std::string dir = self.dli_fname;
        const size_t slash = dir.rfind('/');
        dir = slash == std::string::npos ? std::string(".") : dir.substr(0, slash);
        std::vector<RtcSource> got;
        std::string all;
        const std::string list = MG_RTC_HDRS;
        for (size_t p = 0; p < list.size();) {
            size_t e = list.find(' ', p);
            if (e == std::string::npos) e = list.size();
            const std::string rel = list.substr(p, e - p);
            p = e + 1;
            if (rel.empty()) continue;
            FILE* f = fopen((dir + "/" + rel).c_str(), "rb");
            if (!f) { reason = "the sources for a run-time compile are missing next to the library: " + dir + "/" + rel; return; }
            RtcSource s;
            s.name = rel.substr(rel.rfind('/') == std::string::npos ? 0 : rel.rfind('/') + 1);
            char buf[65536];
            size_t n;
            while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.text.append(buf, n);
            fclose(f);
            all += s.text;
            got.push_back(std::move(s));
        }
        if (posix_cksum(all) != MG_RTC_HDR_CKSUM) { reason = "the headers in " + dir + " are not the ones this library was built from"; return; }
        sources = std::move(got);
    });
    if (sources.empty() && why) *why = reason;
    return sources.empty() ? nullptr : &sources;
}

// ---- libhiprtc, by name ------------------------------------------------------------------------------------------------------
typedef struct _mgHiprtcProgram* RtcProgram;
struct Hiprtc {
    int (*CreateProgram)(RtcProgram*, const char*, const char*, int, const char* const*, const char* const*);
    int (*AddNameExpression)(RtcProgram, const char*);
    int (*CompileProgram)(RtcProgram, int, const char* const*);
    int (*GetLoweredName)(RtcProgram, const char*, const char**);
    int (*GetProgramLogSize)(RtcProgram, size_t*);
    int (*GetProgramLog)(RtcProgram, char*);
    int (*GetCodeSize)(RtcProgram, size_t*);
    int (*GetCode)(RtcProgram, char*);
    int (*DestroyProgram)(RtcProgram*);
    int (*Version)(int*, int*);
    int major, minor;
};

std::mutex g_mutex;      // everything below the C ABI here runs under it: compiles are rare and long

// the copy already in the process (the one the HIP runtime in use was built with), then the development name, then the versioned ones
const Hiprtc* hiprtc(std::string* why) {
    static Hiprtc rtc;
    static int state = 0;      // 0 not tried, 1 loaded, -1 absent
    static std::string reason;
    if (state == 0) {
        static const char* const names[] = {"libhiprtc.so", "libhiprtc.so.7", "libhiprtc.so.6", "libhiprtc.so.5"};
        void* h = nullptr;
        for (const char* n : names) if (!h) h = dlopen(n, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
        for (const char* n : names) if (!h) h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        state = -1;
        if (!h) {
            reason = "libhiprtc could not be loaded (libhiprtc.so, libhiprtc.so.7 ... .5): ";
            const char* e = dlerror();
            reason += e ? e : "not found";
        } else {
            bool ok = true;
#define MG_RTC_SYM(f) ok = ok && (*(void**)&rtc.f = dlsym(h, "hiprtc" #f)) != nullptr;
            MG_RTC_SYM(CreateProgram) MG_RTC_SYM(AddNameExpression) MG_RTC_SYM(CompileProgram) MG_RTC_SYM(GetLoweredName)
            MG_RTC_SYM(GetProgramLogSize) MG_RTC_SYM(GetProgramLog) MG_RTC_SYM(GetCodeSize) MG_RTC_SYM(GetCode)
            MG_RTC_SYM(DestroyProgram) MG_RTC_SYM(Version)
#undef MG_RTC_SYM
            if (!ok) reason = "the libhiprtc in this process lacks a hiprtc* entry point";
            else {
                rtc.major = rtc.minor = 0;
                rtc.Version(&rtc.major, &rtc.minor);
                state = 1;
            }
        }
    }
    if (state != 1 && why) *why = reason;
    return state == 1 ? &rtc : nullptr;
}

// ---- the code object: where its kernel descriptor says how much LDS and scratch the kernel takes ------------------------------------
uint32_t fnv1a(const void* p, size_t n, uint32_t h = 2166136261u) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 16777619u;
    return h;
}

template <class T>
bool rd(const std::vector<char>& b, size_t off, T* out) {
    if (off > b.size() || sizeof(T) > b.size() - off) return false;
    memcpy(out, b.data() + off, sizeof(T));
    return true;
}

// `code`: an ELF64 code object (or a clang offload bundle around one).  The kernel descriptor — symbol "<kernel>.kd", 64 bytes —
// starts with group_segment_fixed_size and private_segment_fixed_size (the figure HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES reports).
bool kernel_descriptor(const std::vector<char>& code, const std::string& kernel, uint32_t* lds, uint32_t* scratch) {
    size_t base = 0;
    static const char kBundle[] = "__CLANG_OFFLOAD_BUNDLE__";
    if (code.size() > 32 && memcmp(code.data(), kBundle, 24) == 0) {
        uint64_t n = 0;
        if (!rd(code, 24, &n)) return false;
        size_t o = 32;
        for (uint64_t i = 0; i < n && i < 64; i++) {
            uint64_t off, size, idlen;
            if (!rd(code, o, &off) || !rd(code, o + 8, &size) || !rd(code, o + 16, &idlen)) return false;
            if (idlen > code.size() || o + 24 > code.size() - idlen) return false;
            const std::string id(code.data() + o + 24, (size_t)idlen);
            o += 24 + (size_t)idlen;
            if (id.compare(0, 4, "host") != 0 && size > 0) { base = (size_t)off; break; }
        }
        if (base == 0) return false;
    }
    auto at = [&](size_t off) { return base + off; };
    unsigned char ident[6];
    if (!rd(code, at(0), &ident) || memcmp(ident, "\177ELF", 4) != 0 || ident[4] != 2 || ident[5] != 1) return false;
    uint64_t shoff;
    uint16_t shentsize, shnum;
    if (!rd(code, at(0x28), &shoff) || !rd(code, at(0x3A), &shentsize) || !rd(code, at(0x3C), &shnum) || shentsize < 64) return false;
    struct Sh { uint32_t type, link; uint64_t addr, off, size, entsize; };
    auto section = [&](unsigned i, Sh* s) {
        const size_t o = at((size_t)shoff + (size_t)i * shentsize);
        return i < shnum && rd(code, o + 4, &s->type) && rd(code, o + 0x10, &s->addr) && rd(code, o + 0x18, &s->off) &&
               rd(code, o + 0x20, &s->size) && rd(code, o + 0x28, &s->link) && rd(code, o + 0x38, &s->entsize);
    };
    const std::string want = kernel + ".kd";
    for (unsigned i = 0; i < shnum; i++) {
        Sh sym, str;
        if (!section(i, &sym) || (sym.type != 2 && sym.type != 11) || sym.entsize < 24 || !section(sym.link, &str)) continue;   // SHT_SYMTAB, SHT_DYNSYM
        for (uint64_t k = 0; k < sym.size / sym.entsize; k++) {
            const size_t o = at((size_t)sym.off + (size_t)(k * sym.entsize));
            uint32_t name;
            uint16_t shndx;
            uint64_t value;
            if (!rd(code, o, &name) || !rd(code, o + 6, &shndx) || !rd(code, o + 8, &value) || name >= str.size) continue;
            const size_t so = at((size_t)str.off + name);
            if (so > code.size() || want.size() + 1 > code.size() - so || memcmp(code.data() + so, want.c_str(), want.size() + 1) != 0) continue;
            Sh home;
            if (!section(shndx, &home) || value < home.addr) return false;
            const size_t kd = at((size_t)(home.off + (value - home.addr)));
            return rd(code, kd, lds) && rd(code, kd + 4, scratch);
        }
    }
    return false;
}

// ---- compiled code: per process, per cache directory ------------------------------------------------------------------------------
struct Compiled {
    std::vector<char> code;
    std::string lowered;       // the kernel's symbol
    uint32_t lds_fixed = 0, scratch = 0;
};
std::map<std::string, Compiled> g_compiled;      // key: parameters, static LDS bytes, arch

struct CacheHeader { char magic[8]; uint32_t code_bytes, name_bytes, checksum, reserved; };      // then the symbol, then the code object
const char kCacheMagic[8] = {'M', 'G', 'S', 'P', 'E', 'C', '1', 0};

std::string cache_path(const char* dir, const Hiprtc& rtc, const std::string& key) {
    char v[48];
    snprintf(v, sizeof v, "hiprtc%d.%d", rtc.major, rtc.minor);
    return std::string(dir) + "/mg_" MG_BUILD_ID "_" + v + "_" + key + ".co";
}

// a file that is not exactly one header, its symbol and its code object with the recorded checksum is not used
bool cache_read(const std::string& path, Compiled* out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    std::vector<char> all;
    char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) all.insert(all.end(), buf, buf + n);
    fclose(f);
    CacheHeader h;
    if (!rd(all, 0, &h) || memcmp(h.magic, kCacheMagic, 8) != 0 || h.name_bytes == 0 || h.name_bytes > 4096 || h.code_bytes == 0) return false;
    if (all.size() != sizeof h + (size_t)h.name_bytes + (size_t)h.code_bytes) return false;
    if (fnv1a(all.data() + sizeof h, all.size() - sizeof h) != h.checksum) return false;
    out->lowered.assign(all.data() + sizeof h, h.name_bytes);
    out->code.assign(all.begin() + sizeof h + h.name_bytes, all.end());
    return kernel_descriptor(out->code, out->lowered, &out->lds_fixed, &out->scratch);
}

// written under a name of this process's own, then renamed: processes that race leave one whole file
void cache_write(const char* dir, const std::string& path, const Compiled& c) {
    mkdir(dir, 0777);      // (one level; an existing directory is fine, anything else shows at fopen)
    char tmp[64];
    snprintf(tmp, sizeof tmp, ".tmp%ld", (long)getpid());
    const std::string t = path + tmp;
    FILE* f = fopen(t.c_str(), "wb");
    if (!f) return;
    CacheHeader h{};
    memcpy(h.magic, kCacheMagic, 8);
    h.code_bytes = (uint32_t)c.code.size();
    h.name_bytes = (uint32_t)c.lowered.size();
    h.checksum = fnv1a(c.code.data(), c.code.size(), fnv1a(c.lowered.data(), c.lowered.size()));
    const bool ok = fwrite(&h, sizeof h, 1, f) == 1 && fwrite(c.lowered.data(), 1, c.lowered.size(), f) == c.lowered.size() &&
                    fwrite(c.code.data(), 1, c.code.size(), f) == c.code.size();
    if (fclose(f) != 0 || !ok || rename(t.c_str(), path.c_str()) != 0) remove(t.c_str());
}

// The translation unit of one instantiation.  hipRTC has no system headers: the fixed-width names, size_t and offsetof the
// headers use come from here (they skip their own #includes under __HIPCC_RTC__).  The sizes of the structs that make up the
// kernel's arguments, as THIS library sees them, are asserted: a layout that differs is a compile error, not a wrong kernarg.
std::string spec_source(const mg::RenderPick& p) {
    char name[96];
    snprintf(name, sizeof name, "mg::render_kernel<%d, %d, %d, %d, %d>", p.vs, p.ts, p.wpb, p.v, p.rm);
    std::string s =
        "typedef __INT8_TYPE__ int8_t; typedef __UINT8_TYPE__ uint8_t; typedef __INT16_TYPE__ int16_t; typedef __UINT16_TYPE__ uint16_t;\n"
        "typedef __INT32_TYPE__ int32_t; typedef __UINT32_TYPE__ uint32_t; typedef __INT64_TYPE__ int64_t; typedef __UINT64_TYPE__ uint64_t;\n"
        "typedef __UINTPTR_TYPE__ uintptr_t; typedef __INTPTR_TYPE__ intptr_t; typedef __SIZE_TYPE__ size_t;\n"
        "#ifndef offsetof\n#define offsetof(t, m) __builtin_offsetof(t, m)\n#endif\n"
        "#include \"mg_render_kernel.h\"\n"
        "static_assert(sizeof(MgConfig) == MG_RTC_SIZEOF_CONFIG && sizeof(MgState) == MG_RTC_SIZEOF_STATE &&\n"
        "              sizeof(mg::RenderLaunch) == MG_RTC_SIZEOF_LAUNCH && sizeof(mg::FusedStep) == MG_RTC_SIZEOF_FUSED,\n"
        "              \"the kernel's argument structs are laid out differently from the library's\");\n"
        "template __global__ void ";
    s += name;
    s += "(MgConfig, MgState, uint8_t*, uint8_t*, uint8_t*, uint8_t*, mg::RenderLaunch, mg::FusedStep);\n";
    return s;
}

std::string kernel_name_of(const mg::RenderPick& p) {
    char name[96];
    snprintf(name, sizeof name, "mg::render_kernel<%d, %d, %d, %d, %d>", p.vs, p.ts, p.wpb, p.v, p.rm);
    return name;
}

// compile `p` for `arch`; lds_static: bytes of LDS compiled in as a static array (0: asked for at the launch)
bool compile(const Hiprtc& rtc, const mg::RenderPick& p, int lds_static, const char* arch, Compiled* out, std::string* why) {
    const std::string src = spec_source(p), expr = "&" + kernel_name_of(p);
    const std::vector<RtcSource>* sources = rtc_sources(why);
    if (!sources) return false;
    std::vector<const char*> names, texts;
    for (const RtcSource& s : *sources) { names.push_back(s.name.c_str()); texts.push_back(s.text.c_str()); }
    RtcProgram prog = nullptr;
    if (rtc.CreateProgram(&prog, src.c_str(), "mg_render_spec.hip", (int)names.size(), texts.data(), names.data()) != 0 || !prog) {
        *why = "hiprtcCreateProgram failed";
        return false;
    }
    char d[5][64];
    snprintf(d[0], 64, "-DMG_RTC_SIZEOF_CONFIG=%zu", sizeof(MgConfig));
    snprintf(d[1], 64, "-DMG_RTC_SIZEOF_STATE=%zu", sizeof(MgState));
    snprintf(d[2], 64, "-DMG_RTC_SIZEOF_LAUNCH=%zu", sizeof(mg::RenderLaunch));
    snprintf(d[3], 64, "-DMG_RTC_SIZEOF_FUSED=%zu", sizeof(mg::FusedStep));
    snprintf(d[4], 64, "-DMG_RTC_LDS_BYTES=%d", lds_static);
    const std::string a = std::string("--offload-arch=") + arch;
    const char* opts[9] = {a.c_str(), "-O3", "-std=c++17", d[0], d[1], d[2], d[3], d[4], nullptr};
    bool ok = rtc.AddNameExpression(prog, expr.c_str()) == 0;
    if (!ok) *why = "hiprtcAddNameExpression failed";
    if (ok && rtc.CompileProgram(prog, lds_static ? 8 : 7, opts) != 0) {
        ok = false;
        size_t n = 0;
        std::string log;
        if (rtc.GetProgramLogSize(prog, &n) == 0 && n > 1) { log.resize(n); rtc.GetProgramLog(prog, &log[0]); }
        const size_t e = log.find("error");
        *why = "hiprtcCompileProgram failed for " + kernel_name_of(p) + ": " + (e == std::string::npos ? log.substr(0, 160) : log.substr(e, 160));
    }
    const char* lowered = nullptr;
    size_t n = 0;
    if (ok && (rtc.GetLoweredName(prog, expr.c_str(), &lowered) != 0 || !lowered || rtc.GetCodeSize(prog, &n) != 0 || n == 0)) {
        ok = false;
        *why = "hipRTC returned no code for " + kernel_name_of(p);
    }
    if (ok) {
        out->lowered = lowered;
        out->code.resize(n);
        ok = rtc.GetCode(prog, out->code.data()) == 0 && kernel_descriptor(out->code, out->lowered, &out->lds_fixed, &out->scratch);
        if (!ok) *why = "the code object of " + kernel_name_of(p) + " has no kernel descriptor for " + out->lowered;
    }
    rtc.DestroyProgram(&prog);
    return ok;
}

// one instantiation's code: this process's memory, the cache directory, the compiler — in that order.  hit: 0 / 1 / 2
const Compiled* compiled_for(const mg::RenderPick& p, int lds_static, const char* arch, const char* cache_dir, int* hit,
                             double* seconds, std::string* why) {
    char k[128];
    snprintf(k, sizeof k, "%s_%d_%d_%d_%d_%d_l%d", arch, p.vs, p.ts, p.wpb, p.v, p.rm, lds_static);
    const std::string key = k;
    *seconds = 0.0;
    auto it = g_compiled.find(key);
    if (it != g_compiled.end()) {
        // (a process that was given a cache directory only now leaves its code there too)
        const Hiprtc* rtc = cache_dir ? hiprtc(nullptr) : nullptr;
        Compiled probe;
        if (rtc && !cache_read(cache_path(cache_dir, *rtc, key), &probe)) cache_write(cache_dir, cache_path(cache_dir, *rtc, key), it->second);
        *hit = 1;
        return &it->second;
    }
    const Hiprtc* rtc = hiprtc(why);
    if (!rtc) return nullptr;
    Compiled c;
    const std::string path = cache_dir ? cache_path(cache_dir, *rtc, key) : std::string();
    if (cache_dir && cache_read(path, &c)) {
        *hit = 2;
    } else {
        const auto t0 = std::chrono::steady_clock::now();
        if (!compile(*rtc, p, lds_static, arch, &c, why)) return nullptr;
        *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        *hit = 0;
        if (cache_dir) cache_write(cache_dir, path, c);      // (a short or corrupt file is replaced by the rename)
    }
    return &(g_compiled[key] = std::move(c));
}

constexpr uint32_t kHandleMagic = 0x4D475350u;      // "MGSP"
struct SpecHandle {
    uint32_t magic;
    int device, want;
    mg::RenderPick pick;
    int lds_static;
    hipModule_t module;
    hipFunction_t fn;
};

void set_reason(MgSpecInfo* info, const std::string& why) {
    snprintf(info->reason, sizeof info->reason, "%s", why.c_str());
}

}  // namespace

namespace mg {

int32_t launch_render_spec(void* handle, const MgConfig& cfg, const MgState& st, uint8_t* obs, hipStream_t s,
                           const FusedStep* fused_step) {
    const SpecHandle* h = static_cast<const SpecHandle*>(handle);
    if (!h || h->magic != kHandleMagic) return MG_E_ARG;
    if (cfg.B <= 0) return MG_OK;
    FusedStep fs{};                 // no step: the raster alone
    fs.action_bytes = 8;
    if (fused_step) fs = *fused_step;
    const RenderWant want = fs.has_ep ? kEpisode : fs.encode_out ? kEncode : kPlain;
    int dev = -1;
    if (want != (RenderWant)h->want || hipGetDevice(&dev) != hipSuccess || dev != h->device) return MG_E_ARG;
    // the handle's instantiation is this configuration's (its workgroup may be a smaller one: the scratch rule, a batch that
    // crossed 4096 envs since) and fits LDS with the handle's workgroup
    RenderPick p;
    if (!render_pick_ideal(cfg, want, &p) || p.vs != h->pick.vs || p.ts != h->pick.ts || p.v != h->pick.v || p.rm != h->pick.rm) return MG_E_ARG;
    if (want == kEncode) fs.enc_ne = render_enc_entries(cfg);
    const size_t lds = render_lds_bytes(cfg, h->pick.wpb, p.rm, p.v, fs.enc_ne);
    if (lds > kRenderLdsMax || (h->lds_static && lds != (size_t)h->lds_static)) return MG_E_ARG;
    RenderLaunch lc;
    const int blocks = render_launch_plan(cfg, h->pick.wpb, p.v, p.rm, lds, &lc);
    MgConfig c = cfg;
    MgState t = st;
    uint8_t* none = nullptr;
    void* args[8] = {&c, &t, &obs, &none, &none, &none, &lc, &fs};
    const hipError_t e = hipModuleLaunchKernel(h->fn, (unsigned)blocks, 1, 1, (unsigned)h->pick.wpb * 64, 1, 1,
                                               h->lds_static ? 0u : (unsigned)lds, s, args, nullptr);
    return e == hipSuccess ? MG_OK : MG_E_LAUNCH;
}

}  // namespace mg

extern "C" {

int32_t mg_spec_info_struct_size(void) { return (int32_t)sizeof(MgSpecInfo); }

int32_t mg_rtc_source(int32_t i, const char** name, const char** text, int32_t* length) {
    std::lock_guard<std::mutex> lock(g_mutex);
    const std::vector<RtcSource>* sources = rtc_sources(nullptr);
    const int32_t n = sources ? (int32_t)sources->size() : 0;
    if (i < 0 || i >= n) return n;
    if (name) *name = (*sources)[i].name.c_str();
    if (text) *text = (*sources)[i].text.c_str();
    if (length) *length = (int32_t)(*sources)[i].text.size();
    return n;
}

int32_t mg_render_specialize(const MgConfig* cfg, int32_t want, uint32_t flags, const char* arch, const char* cache_dir,
                             void** handle, MgSpecInfo* info) {
    if (!cfg || !info || want < 0 || want > 2 || (flags & ~(uint32_t)MG_SPEC_COMPILE_ONLY)) return MG_E_ARG;
    const bool compile_only = (flags & MG_SPEC_COMPILE_ONLY) != 0;
    if (compile_only ? !arch : !handle) return MG_E_ARG;
    if (cfg->B < 1 || cfg->n_agents < 1 || cfg->n_agents > MG_MAX_AGENTS || cfg->view_size < 1 || cfg->view_size > MG_MAX_VIEW ||
        cfg->tile_size < 1 || cfg->tile_size > 64 || cfg->cells_stride < 0 || cfg->n_tiles < 0 || cfg->n_obj < 1 || cfg->n_obj > MG_MAX_OBJ)
        return MG_E_ARG;
    if (arch && (strlen(arch) > 32 || strspn(arch, "abcdefghijklmnopqrstuvwxyz0123456789:+-") != strlen(arch))) return MG_E_ARG;
    memset(info, 0, sizeof *info);
    if (handle) *handle = nullptr;
    mg::RenderPick p;
    if (!mg::render_pick_ideal(*cfg, (mg::RenderWant)want, &p)) {
        // why: render_pick_ideal's own conditions, in its order (what is left when the table has an answer for this `want`: the
        // table's instantiation is the ideal one)
        mg::RenderPick t, plain;
        const bool fits = mg::render_pick(*cfg, mg::kPlain, &plain), have = mg::render_pick(*cfg, (mg::RenderWant)want, &t);
        const char* why = cfg->view_size < 3   ? "views under 3 are not specialised"
                          : cfg->prestige_mask ? "'prestige' agents are not specialised"
                          : !fits              ? "the configuration does not fit the observation kernel's LDS"
                          : plain.v != 0       ? "a grid or an atlas that is read in place is not specialised"
                          : have               ? "the table's instantiation already has this view and this tile size compiled in"
                                               : "the fused encode's table does not fit LDS beside four waves of scratch (or object ids and agent marks do not share a byte)";
        info->table_is_ideal = (cfg->view_size >= 3 && !cfg->prestige_mask && fits && plain.v == 0 && have) ? 1 : 0;
        if (have) {
            snprintf(info->kernel_name, sizeof info->kernel_name, "%s", kernel_name_of(t).c_str());
            info->vs = t.vs; info->ts = t.ts; info->wpb = t.wpb; info->v = t.v; info->rm = t.rm; info->lds_bytes = t.lds;
        }
        set_reason(info, why);
        return MG_E_UNSUPPORTED;
    }
    std::lock_guard<std::mutex> lock(g_mutex);
    int dev = -1;
    std::string arch_s;
    if (arch) arch_s = arch;
    if (!compile_only) {
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return MG_E_LAUNCH;
        if (!arch) arch_s = prop.gcnArchName;
        const size_t colon = arch_s.find(':');      // "gfx950:sramecc+:xnack-" -> the processor alone, as the library itself is built
        if (!arch && colon != std::string::npos) arch_s.resize(colon);
    }
    const int enc_ne = want == 1 ? mg::render_enc_entries(*cfg) : 0;
    std::string why;
    // The scratch rule: an instantiation that spills registers (a private segment) is not launched — its spills would be VMEM
    // traffic in the middle of the store run —: the next smaller workgroup gives the compiler more registers per lane.
    for (;;) {
        const size_t lds = mg::render_lds_bytes(*cfg, p.wpb, p.rm, p.v, enc_ne);
        if (lds <= mg::kRenderLdsMax) {
            p.lds = (int)lds;
            // workgroups over 64 KiB of LDS: the size is compiled in as a static array (the table's launcher asks with
            // hipFuncSetAttribute, which takes a host function, not a module's)
            const int lds_static = lds > 64 * 1024 ? (int)lds : 0;
            int hit = 0;
            double seconds = 0.0;
            const Compiled* c = compiled_for(p, lds_static, arch_s.c_str(), cache_dir, &hit, &seconds, &why);
            if (!c) { set_reason(info, why); return MG_E_UNSUPPORTED; }
            snprintf(info->kernel_name, sizeof info->kernel_name, "%s", kernel_name_of(p).c_str());
            info->vs = p.vs; info->ts = p.ts; info->wpb = p.wpb; info->v = p.v; info->rm = p.rm;
            info->lds_bytes = p.lds;
            info->lds_static = lds_static ? 1 : 0;
            info->scratch_bytes = (int32_t)c->scratch;
            info->code_bytes = (int32_t)c->code.size();
            info->cache_hit = hit;
            info->compile_seconds += seconds;
            if (lds_static && c->lds_fixed < (uint32_t)lds_static) { set_reason(info, "the code object does not carry its static LDS"); return MG_E_UNSUPPORTED; }
            if (c->scratch == 0) {
                if (compile_only) return MG_OK;
                SpecHandle* h = new SpecHandle{kHandleMagic, dev, want, p, lds_static, nullptr, nullptr};
                int local = -1;
                if (hipModuleLoadData(&h->module, c->code.data()) != hipSuccess ||
                    hipModuleGetFunction(&h->fn, h->module, c->lowered.c_str()) != hipSuccess ||
                    hipFuncGetAttribute(&local, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, h->fn) != hipSuccess) {
                    if (h->module) (void)hipModuleUnload(h->module);
                    delete h;
                    set_reason(info, "loading the code object of " + kernel_name_of(p) + " failed");
                    return MG_E_LAUNCH;
                }
                info->scratch_bytes = local;
                if (local == 0) { *handle = h; return MG_OK; }
                (void)hipModuleUnload(h->module);      // (the loader sees a private segment the descriptor did not show: the same rule)
                delete h;
            }
        }
        if (p.wpb <= 4) break;
        p.wpb >>= 1;
    }
    set_reason(info, kernel_name_of(p) + " needs " + std::to_string(info->scratch_bytes) + " bytes of scratch memory per lane even with 4-wave workgroups");
    return MG_E_UNSUPPORTED;
}

int32_t mg_render_spec_release(void* handle) {
    SpecHandle* h = static_cast<SpecHandle*>(handle);
    if (!h) return MG_OK;
    if (h->magic != kHandleMagic) return MG_E_ARG;
    // on the handle's device (a module belongs to the context it was loaded in)
    int cur = -1;
    hipError_t e = hipGetDevice(&cur);
    if (e == hipSuccess && cur != h->device) e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipModuleUnload(h->module);
    if (cur >= 0 && cur != h->device) (void)hipSetDevice(cur);
    h->magic = 0;
    delete h;
    return e == hipSuccess ? MG_OK : MG_E_LAUNCH;
}

}  // extern "C"
