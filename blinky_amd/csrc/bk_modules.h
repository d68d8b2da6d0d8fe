// bk_modules.h -- from generated source text to loadable code: GPU code objects (memory cache -> disk cache -> hiprtc) and the host
// module (the same translation unit compiled by the system's C++ compiler and dlopen'ed).
#pragma once

#include <future>
#include <memory>
#include <string>
#include <vector>
#include <dlfcn.h>
#include <unistd.h>

#include "bk_build_params.h"
#include "bk_internal.h"

// a compiled lens module (or why there is none): what the memory cache, the disk cache or hiprtc hands back
struct CodeResult {
    int rc = BK_OK;
    std::string log;
    std::shared_ptr<std::vector<char>> code;
    bool from_disk = false;
};

struct HostModule {
    void *dl = nullptr;
    int fd = -1;                       // the descriptor the object was verified and loaded through; kept open: see load_host_module
    void (*inverse)(const BkBuildParams *, const unsigned int *, int, unsigned long, unsigned int *, unsigned char *, unsigned short *, int *, int *) = nullptr;
    void (*corners)(const BkBuildParams *, const unsigned int *, int, unsigned long, int *, int *, unsigned char *, int *) = nullptr;
    void (*texel_owns)(const BkBuildParams *, const unsigned int *, int, unsigned long, unsigned char *) = nullptr;
    int (*inverse_scan)(const BkBuildParams *, unsigned int *, unsigned char *, unsigned short *, int *) = nullptr;
    ~HostModule() { if (dl) dlclose(dl); if (fd >= 0) close(fd); }
};
using HostModuleP = std::shared_ptr<HostModule>;

#pragma GCC visibility push(hidden)      // (what crosses between the library's own translation units is not part of its surface)

// memory / disk lookups only (cheap); empty result when the source still has to be compiled
CodeResult cached_code(const std::string &source, const std::string &arch);
// one compilation per (source, arch) and process: the stripe contexts of a bk_multi build the same lens side by side
CodeResult compile_code(const std::string &source, const std::string &arch);
// a compilation nobody waits for any more: kept until it is done instead of being waited for here; `f` comes back empty
void park_compile(std::shared_future<CodeResult> &f);

// the host module for this generated source: ready -> returned; otherwise a compile is started (once) and nullptr returned,
// unless `wait`.  Never throws; nullptr simply means "use the interpreter".
HostModuleP host_module_for(const std::string &source, bool wait);

#pragma GCC visibility pop
