// bk_codecache.cpp -- the on-disk cache of compiled code: its directory, SHA-256, and the checks a file passes before it is loaded.
#include "bk_codecache.h"

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/blinky_hip.h"

// Optional on-disk cache of compiled lens modules (opt-in: BLINKY_HIP_CACHE=<directory>).  hiprtc takes
// 0.2-1.1 s per lens, which the engine would feel as a hitch on every first `f_lens`; a code object is keyed by
// FNV-1a-64 over the generated source, the embedded headers, the target arch and the library version.
uint64_t bk::fnv1a64(const void *data, size_t n, uint64_t h)
{
    const unsigned char *p = (const unsigned char *)data;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}

// The directory bk_set_cache_dir() named.  Threads started with std::async (a lens or host-module compile nobody waits for any more)
// ask for it, and at process exit one of them can still be running while static objects are destroyed - in an order that is not
// fixed between this translation unit and theirs.  So this state is never destroyed: made on first use and leaked on purpose.
namespace {
struct CacheDirState {
    std::mutex mutex;
    std::string dir;
    bool set = false;
};
CacheDirState &cache_dir_state()
{
    static CacheDirState *const state = new CacheDirState;
    return *state;
}
}  // namespace

extern "C" int bk_set_cache_dir(const char *dir)
{
    CacheDirState &s = cache_dir_state();
    std::lock_guard<std::mutex> lock(s.mutex);
    s.dir = dir ? dir : "";
    s.set = dir != nullptr;              // NULL: back to the environment / default location
    return BK_OK;
}

namespace bk {

std::string cache_dir()
{
    {
        CacheDirState &s = cache_dir_state();
        std::lock_guard<std::mutex> lock(s.mutex);
        if (s.set) return s.dir;
    }
    if (const char *e = getenv("BLINKY_HIP_CACHE")) return (!*e || !strcmp(e, "off")) ? std::string() : std::string(e);
    if (const char *x = getenv("XDG_CACHE_HOME")) if (*x) return std::string(x) + "/blinky_hip";
    if (const char *h = getenv("HOME")) if (*h) return std::string(h) + "/.cache/blinky_hip";
    return std::string();
}

// ---- what may be loaded from the cache ---------------------------------------------------------------------------------
// A cached object is CODE - GPU code objects, and since round 3 host shared objects that are dlopen()ed into the engine - so the
// cache is only ever a directory that belongs to the user and that nobody else can write to, the files in it likewise, opened
// without following links and checked through the descriptor that is then read / loaded (no check-then-open window).  Names
// carry 128 bits of a SHA-256 over everything the object was built from (source, embedded headers, target / compiler + its
// size and modification time, flags, library version): no collisions to speak of, no stale objects after an upgrade.  Every
// file ends in a trailer - "BKSHA256" + the SHA-256 of what precedes it - that is verified before the object is used: a torn
// or corrupted file is a cache miss, not wrong lensmap entries.  (The digest is not a signature: against somebody who can
// write to the directory only the ownership checks help, which is why a directory that fails them is not used at all.)
static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
void Sha256::block(const unsigned char *p)
{
    static const uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
        0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
        0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
        0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
        0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
        0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t w[64];
    for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; ++i) {
        const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
        w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; ++i) {
        const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}
void Sha256::update(const void *data, size_t n)
{
    const unsigned char *p = (const unsigned char *)data;
    len += n;
    while (n) {
        const size_t take = std::min(n, sizeof buf - fill);
        memcpy(buf + fill, p, take);
        fill += take; p += take; n -= take;
        if (fill == 64) { block(buf); fill = 0; }
    }
}
void Sha256::finish(unsigned char out[32])
{
    const uint64_t bits = len * 8;
    const unsigned char one = 0x80, zero = 0;
    update(&one, 1);
    while (fill != 56) update(&zero, 1);
    unsigned char l[8];
    for (int i = 0; i < 8; ++i) l[i] = (unsigned char)(bits >> (56 - 8 * i));
    update(l, 8);
    for (int i = 0; i < 8; ++i) { out[4 * i] = (unsigned char)(h[i] >> 24); out[4 * i + 1] = (unsigned char)(h[i] >> 16); out[4 * i + 2] = (unsigned char)(h[i] >> 8); out[4 * i + 3] = (unsigned char)h[i]; }
}
std::string hex128(Sha256 &s)
{
    unsigned char d[32];
    s.finish(d);
    char out[33];
    for (int i = 0; i < 16; ++i) snprintf(out + 2 * i, 3, "%02x", d[i]);
    return out;
}
static const char kTrailerMagic[8] = {'B', 'K', 'S', 'H', 'A', '2', '5', '6'};
void trailer_of(const void *data, size_t n, unsigned char out[40])
{
    Sha256 s;
    s.update(data, n);
    memcpy(out, kTrailerMagic, 8);
    s.finish(out + 8);
}

bool cache_dir_ok(const std::string &dir, bool create)
{
    if (dir.empty()) return false;
    struct stat st;
    if (lstat(dir.c_str(), &st) != 0) {
        if (!create) return false;
        const size_t cut = dir.rfind('/');
        if (cut != std::string::npos && cut > 0)
            for (size_t i = 1; i <= cut; ++i)
                if (i == cut || dir[i] == '/') (void)mkdir(dir.substr(0, i).c_str(), 0755);        // (the way there: ordinary directories)
        if (mkdir(dir.c_str(), 0700) != 0 && errno != EEXIST) return false;
        if (lstat(dir.c_str(), &st) != 0) return false;
    }
    return S_ISDIR(st.st_mode) && st.st_uid == geteuid() && (st.st_mode & (S_IWGRP | S_IWOTH)) == 0;
}
int open_checked(const std::string &path)
{
    const int fd = open(path.c_str(), O_RDONLY | O_NOFOLLOW | O_CLOEXEC);
    if (fd < 0) return -1;
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_uid != geteuid() || (st.st_mode & (S_IWGRP | S_IWOTH)) != 0) { close(fd); return -1; }
    return fd;
}
bool read_verified(int fd, std::vector<char> *out)
{
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size <= 40) return false;
    out->resize((size_t)st.st_size);
    size_t got = 0;
    while (got < out->size()) {
        const ssize_t n = pread(fd, out->data() + got, out->size() - got, (off_t)got);
        if (n <= 0) { if (n < 0 && errno == EINTR) continue; return false; }
        got += (size_t)n;
    }
    unsigned char want[40];
    trailer_of(out->data(), out->size() - 40, want);
    if (memcmp(want, out->data() + out->size() - 40, 40) != 0) return false;
    out->resize(out->size() - 40);
    return true;
}
bool write_all(int fd, const void *data, size_t n)
{
    const char *p = (const char *)data;
    while (n) {
        const ssize_t w = write(fd, p, n);
        if (w <= 0) { if (w < 0 && errno == EINTR) continue; return false; }
        p += w; n -= (size_t)w;
    }
    return true;
}

bool load_sealed(const std::string &path, std::vector<char> *bytes)
{
    if (path.empty() || !cache_dir_ok(path.substr(0, path.rfind('/')), false)) return false;
    const int fd = open_checked(path);
    if (fd < 0) return false;
    const bool ok = read_verified(fd, bytes);
    close(fd);
    return ok;
}
void store_sealed(const std::string &path, const std::vector<char> &bytes)
{
    if (path.empty() || !cache_dir_ok(path.substr(0, path.rfind('/')), true)) return;       // a cache that cannot be trusted / written is simply not used
    const std::string tmp = path + ".tmp" + std::to_string((long long)getpid());
    const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0600);
    if (fd < 0) return;
    unsigned char tr[40];
    trailer_of(bytes.data(), bytes.size(), tr);
    const bool ok = write_all(fd, bytes.data(), bytes.size()) && write_all(fd, tr, sizeof tr);
    close(fd);
    if (!ok || rename(tmp.c_str(), path.c_str()) != 0) remove(tmp.c_str());
}
// (a host module: the trailer goes behind the ELF image - the loader maps by program headers: trailing bytes are not looked at)
bool seal_in_place(const std::string &path)
{
    std::vector<char> img;
    const int fd = open(path.c_str(), O_RDWR | O_NOFOLLOW | O_CLOEXEC);
    struct stat st;
    bool sealed = false;
    if (fd >= 0 && fstat(fd, &st) == 0 && st.st_size > 0) {
        img.resize((size_t)st.st_size);
        if (pread(fd, img.data(), img.size(), 0) == (ssize_t)img.size()) {
            unsigned char tr[40];
            trailer_of(img.data(), img.size(), tr);
            sealed = lseek(fd, 0, SEEK_END) >= 0 && write_all(fd, tr, sizeof tr) && fchmod(fd, 0600) == 0;
        }
    }
    if (fd >= 0) close(fd);
    return sealed;
}

}  // namespace bk
