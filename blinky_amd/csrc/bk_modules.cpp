// bk_modules.cpp -- generated source text -> loadable code: hiprtc and the code caches, the host-module compiler (bk_modules.h).
#include <hip/hiprtc.h>

#include <cerrno>
#include <chrono>
#include <cstring>
#include <map>
#include <mutex>
#include <dlfcn.h>
#include <fcntl.h>
#include <spawn.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include "bk_codecache.h"
#include "bk_emit.h"
#include "bk_modules.h"

using namespace bk;
extern char **environ;

static std::string cache_path(const std::string &source, const std::string &arch)
{
    const std::string dir = cache_dir();
    if (dir.empty()) return std::string();
    Sha256 h;
    h.update(source);
    for (int i = 0; i < bk::kNumEmbeddedHeaders; ++i) h.update(std::string(bk::kEmbeddedHeaders[i].text));
    h.update(arch);
    h.update(std::string(bk_version()));
    h.update(std::string("-O3 -std=c++17 -ffp-contract=off"));
    return dir + "/bk_lens_" + hex128(h) + ".hsaco";
}

// ---- code objects: memory cache -> disk cache -> hiprtc ------------------------------------------------------------
static std::mutex g_rtc_mutex;                                   // hiprtc + the memory cache
static std::map<uint64_t, std::shared_ptr<std::vector<char>>> g_rtc_cache;

static uint64_t code_key(const std::string &source, const std::string &arch)
{
    return fnv1a64(arch.data(), arch.size(), fnv1a64(source.data(), source.size()));
}

CodeResult cached_code(const std::string &source, const std::string &arch)
{
    CodeResult r;
    std::lock_guard<std::mutex> lock(g_rtc_mutex);
    const bool use_mem = !bk::g_debug.no_memcache;                  // (tests of the disk cache switch the memory cache off)
    auto hit = g_rtc_cache.find(code_key(source, arch));
    if (use_mem && hit != g_rtc_cache.end()) { r.code = hit->second; return r; }
    std::vector<char> code;
    if (load_sealed(cache_path(source, arch), &code)) {
        r.code = std::make_shared<std::vector<char>>(std::move(code));
        r.from_disk = true;
        if (g_rtc_cache.size() >= 64) g_rtc_cache.clear();          // (a long session cycling through many lenses)
        g_rtc_cache[code_key(source, arch)] = r.code;
    }
    return r;
}

CodeResult compile_code(const std::string &source, const std::string &arch)
{
    CodeResult r = cached_code(source, arch);
    if (r.code) return r;
    std::lock_guard<std::mutex> lock(g_rtc_mutex);
    auto hit = g_rtc_cache.find(code_key(source, arch));
    if (hit != g_rtc_cache.end() && !bk::g_debug.no_memcache) { r.code = hit->second; return r; }   // another thread was faster
    std::vector<const char *> hnames, htexts;
    for (int i = 0; i < bk::kNumEmbeddedHeaders; ++i) {
        hnames.push_back(bk::kEmbeddedHeaders[i].name);
        htexts.push_back(bk::kEmbeddedHeaders[i].text);
    }
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, source.c_str(), "bk_lens_build.hip", (int)hnames.size(), htexts.data(), hnames.data()) != HIPRTC_SUCCESS) {
        r.rc = BK_E_HIP; r.log = "hiprtcCreateProgram failed";
        return r;
    }
    const char *opts[] = {arch.c_str(), "-O3", "-std=c++17", "-ffp-contract=off"};
    if (hiprtcCompileProgram(prog, 4, opts) != HIPRTC_SUCCESS) {
        size_t n = 0;
        hiprtcGetProgramLogSize(prog, &n);
        std::string log(n, 0);
        if (n) hiprtcGetProgramLog(prog, &log[0]);
        hiprtcDestroyProgram(&prog);
        r.rc = BK_E_HIP; r.log = "hiprtc failed to compile the lens kernels: " + log;
        return r;
    }
    size_t cs = 0;
    hiprtcGetCodeSize(prog, &cs);
    r.code = std::make_shared<std::vector<char>>(cs);
    hiprtcGetCode(prog, r.code->data());
    hiprtcDestroyProgram(&prog);
    store_sealed(cache_path(source, arch), *r.code);
    if (g_rtc_cache.size() >= 64) g_rtc_cache.clear();
    g_rtc_cache[code_key(source, arch)] = r.code;
    return r;
}


// ---- host module: the generated lens code compiled for the HOST ----------------------------------------------------
// The entries a build flags are re-derived on the platform libm.  The script interpreter does that at 4-10 us per entry;
// the very translation unit hiprtc receives, compiled by the system's C++ compiler against the platform libm
// (bk_hostmod_bkm.h in place of bkm.h, bk_hostmod_driver.inc appended) and dlopen'ed, does it in a fraction of a
// microsecond - the same per-entry functions the kernels call, the same IEEE operations in the same order, libm calls
// resolved in this process's libm.  The compiler runs on another thread and its output is cached next to the device code
// objects; until it is there (or if the machine has no compiler) the interpreter answers, so nothing ever waits for it and
// results are the same either way (tests/test_hostmod.py holds the two against each other entry for entry).
static std::mutex g_hostmod_mutex;
static std::map<uint64_t, HostModuleP> g_hostmods;                          // ready (nullptr = failed: do not try again)
static std::map<uint64_t, std::shared_future<HostModuleP>> g_hostmod_jobs;  // compiling
static int g_hostmod_enabled = 1;                                           // bk_set_host_compile

extern "C" int bk_set_host_compile(int on)
{
    std::lock_guard<std::mutex> lock(g_hostmod_mutex);
    g_hostmod_enabled = on != 0;
    return BK_OK;
}

// the C++ compiler to run: $BLINKY_HIP_HOSTCXX ("off" / "" = none), else the first of c++ / g++ / clang++ on $PATH, else ROCm's clang
static std::string host_compiler()
{
    auto on_path = [](const char *name) -> std::string {
        const char *path = getenv("PATH");
        if (!path) return std::string();
        std::string p(path);
        for (size_t b = 0; b <= p.size();) {
            size_t e = p.find(':', b);
            if (e == std::string::npos) e = p.size();
            const std::string cand = p.substr(b, e - b) + "/" + name;
            if (e > b && access(cand.c_str(), X_OK) == 0) return cand;
            b = e + 1;
        }
        return std::string();
    };
    if (const char *e = getenv("BLINKY_HIP_HOSTCXX")) {
        if (!*e || !strcmp(e, "off")) return std::string();
        if (strchr(e, '/')) return access(e, X_OK) == 0 ? std::string(e) : std::string();
        return on_path(e);
    }
    for (const char *name : {"c++", "g++", "clang++"}) { std::string c = on_path(name); if (!c.empty()) return c; }
    for (const char *abs : {"/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/bin/amdclang++"}) if (access(abs, X_OK) == 0) return abs;
    return std::string();
}

static const char *embedded_text(const char *name)
{
    for (int i = 0; i < bk::kNumEmbeddedHeaders; ++i) if (!strcmp(bk::kEmbeddedHeaders[i].name, name)) return bk::kEmbeddedHeaders[i].text;
    return "";
}

// the shared object is loaded THROUGH the descriptor it was checked and verified on (/proc/self/fd): what is mapped is what was read
static HostModuleP load_host_module(const std::string &so)
{
    const int fd = open_checked(so);
    if (fd < 0) return nullptr;
    std::vector<char> content;
    if (!read_verified(fd, &content)) { close(fd); return nullptr; }
    // (the descriptor stays open as long as the module lives: the dynamic loader knows an object by the NAME it was opened under, and a
    //  descriptor number that was closed and handed out again would make "/proc/self/fd/N" answer with the module loaded before)
    const std::string via = "/proc/self/fd/" + std::to_string(fd);
    void *dl = dlopen(via.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!dl) { close(fd); return nullptr; }
    HostModuleP m = std::make_shared<HostModule>();
    m->dl = dl;
    m->fd = fd;
    auto abi = (int (*)(void))dlsym(dl, "bk_hostmod_abi");
    m->inverse = (decltype(m->inverse))dlsym(dl, "bk_hostmod_inverse");
    m->corners = (decltype(m->corners))dlsym(dl, "bk_hostmod_corners");
    m->texel_owns = (decltype(m->texel_owns))dlsym(dl, "bk_hostmod_texel_owns");
    m->inverse_scan = (decltype(m->inverse_scan))dlsym(dl, "bk_hostmod_inverse_scan");
    if (!abi || abi() != 5 + (int)sizeof(BkBuildParams) * 16 || !m->inverse || !m->corners || !m->texel_owns || !m->inverse_scan) return nullptr;
    return m;
}

static bool write_text(const std::string &path, const std::string &text)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    fclose(f);
    return ok;
}

// compile `source` for the host with `cxx`; the shared object ends up at `so_path` (atomically)
static HostModuleP compile_host_module(const std::string &source, const std::string &cxx, const std::string &so_path)
{
    // a scratch directory nobody else can have prepared: mkdtemp (0700, fails if the name exists) inside the checked cache directory
    std::string tmpl = so_path.substr(0, so_path.rfind('/')) + "/build.XXXXXX";
    if (!mkdtemp(&tmpl[0])) return nullptr;
    const std::string dir = tmpl;
    bool ok = write_text(dir + "/bkm.h", embedded_text("bk_hostmod_bkm.h"));
    for (const char *h : {"bk_build_params.h", "bk_device_rt.h", "bk_build_kernels.h"}) ok = ok && write_text(dir + "/" + h, embedded_text(h));
    const std::string unit = std::string("#define BK_HOST_MODULE 1\n#define __device__\n#define __forceinline__ inline\n") + source + "\n" +
                             embedded_text("bk_hostmod_driver.inc");
    ok = ok && write_text(dir + "/unit.cpp", unit);
    HostModuleP m;
    if (ok) {
        const std::string out = dir + "/unit.so", inc = "-I" + dir, src = dir + "/unit.cpp";
        const char *argv[] = {cxx.c_str(), "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin", "-fno-fast-math", "-fPIC", "-shared", "-w",
                              inc.c_str(), "-o", out.c_str(), src.c_str(), nullptr};
        pid_t pid = 0;
        posix_spawn_file_actions_t fa;
        posix_spawn_file_actions_init(&fa);
        posix_spawn_file_actions_addopen(&fa, 1, "/dev/null", O_WRONLY, 0);
        posix_spawn_file_actions_addopen(&fa, 2, "/dev/null", O_WRONLY, 0);
        int status = -1;
        if (posix_spawn(&pid, cxx.c_str(), &fa, nullptr, const_cast<char *const *>(argv), environ) == 0) {
            while (waitpid(pid, &status, 0) < 0 && errno == EINTR) {}
        }
        posix_spawn_file_actions_destroy(&fa);
        if (status == 0 && seal_in_place(out) && rename(out.c_str(), so_path.c_str()) == 0) m = load_host_module(so_path);
    }
    for (const char *f : {"bkm.h", "bk_build_params.h", "bk_device_rt.h", "bk_build_kernels.h", "unit.cpp", "unit.so"}) remove((dir + "/" + f).c_str());
    rmdir(dir.c_str());
    return m;
}

HostModuleP host_module_for(const std::string &source, bool wait)
{
    // (source + everything it is compiled with; the headers' part once - they are 100 KB, and this runs in every build that flagged a pixel)
    static const uint64_t headers_key = [] {
        uint64_t k = 1469598103934665603ull;
        for (const char *h : {"bk_hostmod_bkm.h", "bk_hostmod_driver.inc", "bk_build_params.h", "bk_device_rt.h", "bk_build_kernels.h"}) {
            const char *t = embedded_text(h);
            k = fnv1a64(t, strlen(t), k);
        }
        return k;
    }();
    const uint64_t key = fnv1a64(source.data(), source.size(), headers_key);
    std::shared_future<HostModuleP> job;
    {
        std::lock_guard<std::mutex> lock(g_hostmod_mutex);
        if (!g_hostmod_enabled) return nullptr;
        auto hit = g_hostmods.find(key);
        if (hit != g_hostmods.end()) return hit->second;
        auto running = g_hostmod_jobs.find(key);
        if (running != g_hostmod_jobs.end()) job = running->second;
        else {
            const std::string cxx = host_compiler();
            if (cxx.empty()) { g_hostmods[key] = nullptr; return nullptr; }
            std::string dir = cache_dir();                                  // next to the device code objects, or a private temp dir
            if (dir.empty()) {                                              // (disk cache off: a directory only this process can have made)
                static std::string private_dir;
                if (private_dir.empty()) {
                    char tmpl[] = "/tmp/blinky_hip_hostmod.XXXXXX";
                    if (!mkdtemp(tmpl)) { g_hostmods[key] = nullptr; return nullptr; }
                    private_dir = tmpl;
                }
                dir = private_dir;
            }
            if (!cache_dir_ok(dir, true)) { g_hostmods[key] = nullptr; return nullptr; }       // (not a directory to load code from: the interpreter answers)
            // the name: 128 bits of a SHA-256 over the source, what it is compiled with (headers, compiler - path, size, modification
            // time - and flags) and the library version
            Sha256 h;
            h.update(source);
            for (const char *hn : {"bk_hostmod_bkm.h", "bk_hostmod_driver.inc", "bk_build_params.h", "bk_device_rt.h", "bk_build_kernels.h"}) h.update(std::string(embedded_text(hn)));
            h.update(cxx);
            { struct stat cst; if (stat(cxx.c_str(), &cst) == 0) { const long long id[2] = {(long long)cst.st_size, (long long)cst.st_mtime}; h.update(id, sizeof id); } }
            h.update(std::string("-O2 -std=c++17 -ffp-contract=off -fno-builtin -fno-fast-math -fPIC -shared"));
            h.update(std::string(bk_version()));
            const std::string so = dir + "/bk_host_" + hex128(h) + ".so";
            {
                HostModuleP m = load_host_module(so);
                if (m) { g_hostmods[key] = m; return m; }
            }
            job = std::async(std::launch::async, [source, cxx, so]() { return compile_host_module(source, cxx, so); }).share();
            g_hostmod_jobs[key] = job;
        }
    }
    if (!wait && job.wait_for(std::chrono::seconds(0)) != std::future_status::ready) return nullptr;
    HostModuleP m = job.get();
    std::lock_guard<std::mutex> lock(g_hostmod_mutex);
    g_hostmods[key] = m;
    g_hostmod_jobs.erase(key);
    return m;
}

// Compilations nobody waits for any more (the lens or zoom changed while hiprtc was still busy, or the context went away).
// A std::async future blocks in its destructor until its thread is done, so a superseded one is not dropped - that would
// stall the render thread for the rest of the compile - but parked here and reaped once ready; its result still lands in the
// memory / disk caches.  (At process exit the list's destructor joins whatever is still running: defined after the caches
// above, it is destroyed before them.)
static std::mutex g_parked_mutex;
static std::vector<std::shared_future<::CodeResult>> g_parked;
void park_compile(std::shared_future<::CodeResult> &f)
{
    std::lock_guard<std::mutex> lock(g_parked_mutex);
    for (size_t i = 0; i < g_parked.size();)
        if (g_parked[i].wait_for(std::chrono::seconds(0)) == std::future_status::ready) { g_parked[i] = g_parked.back(); g_parked.pop_back(); }
        else ++i;
    if (f.valid() && f.wait_for(std::chrono::seconds(0)) != std::future_status::ready) g_parked.push_back(f);
    f = std::shared_future<::CodeResult>();
}
