// codecache_check.cpp -- stand-alone check of what the code cache trusts (blinky_amd/csrc/bk_codecache.cpp): links that unit alone, no
// HIP, no Python; works inside a mkdtemp directory.  Prints what failed and exits non-zero.  `make sanitize` builds it with
// AddressSanitizer + UndefinedBehaviorSanitizer.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <fcntl.h>
#include <ftw.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../blinky_amd/csrc/bk_codecache.h"
#include "../../include/blinky_hip.h"

static int g_failed = 0;
#define CHECK(cond, ...)                                           \
    do {                                                           \
        if (!(cond)) {                                             \
            ++g_failed;                                            \
            fprintf(stderr, "codecache_check: FAILED %s: ", #cond); \
            fprintf(stderr, __VA_ARGS__);                          \
            fprintf(stderr, "\n");                                 \
        }                                                          \
    } while (0)

static std::string sha256_hex(const void *data, size_t n)
{
    bk::Sha256 s;
    s.update(data, n);
    unsigned char d[32];
    s.finish(d);
    char out[65];
    for (int i = 0; i < 32; ++i) snprintf(out + 2 * i, 3, "%02x", d[i]);
    return out;
}

static void check_sha256()
{
    const std::string two_blocks = "abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", million(1000000, 'a');
    const struct { const std::string msg; const char *want; } cases[] = {       // (digests: Python's hashlib)
        {"", "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"},
        {"abc", "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"},
        {two_blocks, "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1"},
        {million, "cdc76e5c9914fb9281a1c7e284d73e67f1809a48a497200e046d39ccc7112cd0"},
    };
    for (const auto &c : cases) {
        const std::string got = sha256_hex(c.msg.data(), c.msg.size());
        CHECK(got == c.want, "SHA-256 of %zu bytes is %s, expected %s", c.msg.size(), got.c_str(), c.want);
    }
    // the same message in uneven pieces
    bk::Sha256 s;
    for (size_t at = 0, step = 1; at < million.size(); at += step, step = step * 3 % 200 + 1) s.update(million.data() + at, std::min(step, million.size() - at));
    unsigned char d[32];
    s.finish(d);
    char hex[65];
    for (int i = 0; i < 32; ++i) snprintf(hex + 2 * i, 3, "%02x", d[i]);
    CHECK(std::string(hex) == cases[3].want, "SHA-256 in pieces is %s", hex);
}

static std::vector<char> content_of(size_t n, unsigned seed)
{
    std::vector<char> v(n);
    for (size_t i = 0; i < n; ++i) { seed = seed * 1664525u + 1013904223u; v[i] = (char)(seed >> 24); }
    return v;
}
static bool loads(const std::string &path, const std::vector<char> &want)
{
    std::vector<char> got;
    return bk::load_sealed(path, &got) && got == want;
}
static bool misses(const std::string &path)
{
    std::vector<char> got;
    return !bk::load_sealed(path, &got);
}
static std::vector<char> raw_read(const std::string &path)
{
    std::vector<char> v;
    if (FILE *f = fopen(path.c_str(), "rb")) {
        char buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
        fclose(f);
    }
    return v;
}
static void raw_write(const std::string &path, const std::vector<char> &v, mode_t mode = 0600)
{
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, mode);
    if (fd < 0 || !bk::write_all(fd, v.data(), v.size())) CHECK(false, "could not write %s", path.c_str());
    if (fd >= 0) { fchmod(fd, mode); close(fd); }
}
static bool exists(const std::string &path) { struct stat st; return lstat(path.c_str(), &st) == 0; }

static void check_round_trip(const std::string &top)
{
    const std::string dir = top + "/a/b/cache", path = dir + "/entry.bin";
    const std::vector<char> bytes = content_of(5000, 1);
    CHECK(misses(path), "a load from a directory that does not exist hit");
    CHECK(!exists(top + "/a"), "a load created directories");
    bk::store_sealed(path, bytes);
    struct stat st;
    CHECK(lstat(dir.c_str(), &st) == 0 && S_ISDIR(st.st_mode) && (st.st_mode & 07777) == 0700, "the cache directory was not made with mode 0700 (mode %o)", (unsigned)(st.st_mode & 07777));
    CHECK(loads(path, bytes), "store then load did not return the same bytes");
    CHECK(raw_read(path).size() == bytes.size() + 40, "a sealed file is not content + 40 bytes");
    const std::vector<char> one(1, 'x');
    bk::store_sealed(dir + "/one.bin", one);
    CHECK(loads(dir + "/one.bin", one), "a one-byte entry did not round-trip");
    CHECK(misses(dir + "/absent.bin"), "an absent entry hit");
    CHECK(misses(std::string()), "the empty path hit");
}

static void check_damage(const std::string &top)
{
    const std::string dir = top + "/damage", path = dir + "/entry.bin";
    const std::vector<char> bytes = content_of(3000, 2);
    bk::store_sealed(path, bytes);
    const std::vector<char> sealed = raw_read(path);
    CHECK(sealed.size() == bytes.size() + 40 && loads(path, bytes), "setting up the damaged-file cases failed");
    if (sealed.size() != bytes.size() + 40) return;
    std::vector<size_t> flips = {0, bytes.size() / 2, bytes.size() - 1};
    for (size_t t = 0; t < 40; ++t) flips.push_back(bytes.size() + t);
    for (size_t at : flips) {
        std::vector<char> v = sealed;
        v[at] = (char)(v[at] ^ 0x01);
        raw_write(path, v);
        CHECK(misses(path), "a file with byte %zu of %zu flipped was loaded", at, sealed.size());
    }
    for (size_t len : {(size_t)0, (size_t)40, (size_t)41, sealed.size() - 1}) {
        raw_write(path, std::vector<char>(sealed.begin(), sealed.begin() + len));
        CHECK(misses(path), "a file truncated to %zu of %zu bytes was loaded", len, sealed.size());
    }
    raw_write(path, sealed);
    CHECK(loads(path, bytes), "the restored file does not load");
    // a symbolic link to a valid file
    const std::string link = dir + "/link.bin";
    CHECK(symlink(path.c_str(), link.c_str()) == 0, "symlink failed");
    CHECK(misses(link), "a symbolic link to a valid file was loaded");
    // a file that somebody else may write to
    for (mode_t mode : {(mode_t)0620, (mode_t)0602, (mode_t)0666}) {
        CHECK(chmod(path.c_str(), mode) == 0, "chmod failed");
        CHECK(misses(path), "a file of mode %o was loaded", (unsigned)mode);
    }
    CHECK(chmod(path.c_str(), 0600) == 0 && loads(path, bytes), "the file does not load with mode 0600 again");
    // a leftover temporary of a store that never finished
    raw_write(path + ".tmp" + std::to_string((long long)getpid()), content_of(100, 3));
    raw_write(path + ".tmp1", content_of(100, 4));
    CHECK(loads(path, bytes), "a leftover .tmp<pid> file shadows the valid entry");
}

static void check_directories(const std::string &top)
{
    const std::vector<char> bytes = content_of(2000, 5);
    // a valid entry in a good directory, which is then opened to others
    const std::string dir = top + "/shared", path = dir + "/entry.bin";
    bk::store_sealed(path, bytes);
    CHECK(loads(path, bytes), "setting up the directory cases failed");
    for (mode_t mode : {(mode_t)0770, (mode_t)0707, (mode_t)0777}) {
        CHECK(chmod(dir.c_str(), mode) == 0, "chmod failed");
        CHECK(!bk::cache_dir_ok(dir, false) && !bk::cache_dir_ok(dir, true), "a directory of mode %o passes", (unsigned)mode);
        CHECK(misses(path), "an entry was loaded from a directory of mode %o", (unsigned)mode);
        bk::store_sealed(dir + "/new.bin", bytes);
        CHECK(!exists(dir + "/new.bin"), "an entry was stored in a directory of mode %o", (unsigned)mode);
    }
    CHECK(chmod(dir.c_str(), 0700) == 0 && loads(path, bytes), "the directory is not used with mode 0700 again");
    // a link to that (good) directory
    const std::string link = top + "/linked";
    CHECK(symlink(dir.c_str(), link.c_str()) == 0, "symlink failed");
    CHECK(!bk::cache_dir_ok(link, false) && !bk::cache_dir_ok(link, true), "a link to a directory passes");
    CHECK(misses(link + "/entry.bin"), "an entry was loaded through a linked directory");
    bk::store_sealed(link + "/new.bin", bytes);
    CHECK(!exists(dir + "/new.bin"), "an entry was stored through a linked directory");
    // a regular file where the directory should be
    raw_write(top + "/plainfile", bytes);
    CHECK(!bk::cache_dir_ok(top + "/plainfile", true), "a regular file passes as a cache directory");
}

static void check_seal_in_place(const std::string &top)
{
    const std::string dir = top + "/seal", path = dir + "/image.bin";
    const std::vector<char> bytes = content_of(4096, 6);
    CHECK(bk::cache_dir_ok(dir, true), "could not make %s", dir.c_str());
    raw_write(path, bytes, 0644);
    CHECK(bk::seal_in_place(path), "seal_in_place failed");
    struct stat st;
    CHECK(stat(path.c_str(), &st) == 0 && (st.st_mode & 07777) == 0600, "a sealed file is not mode 0600");
    CHECK(loads(path, bytes), "a file sealed in place does not load");
    CHECK(!bk::seal_in_place(dir + "/absent.bin"), "sealing an absent file succeeded");
}

static void check_cache_dir()
{
    setenv("BLINKY_HIP_CACHE", "/somewhere/else", 1);
    CHECK(bk::cache_dir() == "/somewhere/else", "BLINKY_HIP_CACHE is not honoured: %s", bk::cache_dir().c_str());
    setenv("BLINKY_HIP_CACHE", "off", 1);
    CHECK(bk::cache_dir().empty(), "BLINKY_HIP_CACHE=off does not disable the cache");
    bk_set_cache_dir("/named/by/the/host");
    CHECK(bk::cache_dir() == "/named/by/the/host", "bk_set_cache_dir is not honoured");
    bk_set_cache_dir("");
    CHECK(bk::cache_dir().empty(), "bk_set_cache_dir(\"\") does not disable the cache");
    bk_set_cache_dir(nullptr);
    unsetenv("BLINKY_HIP_CACHE");
    setenv("XDG_CACHE_HOME", "/xdg", 1);
    CHECK(bk::cache_dir() == "/xdg/blinky_hip", "XDG_CACHE_HOME is not honoured");
}

int main()
{
    umask(022);
    char tmpl[] = "/tmp/bk_codecache_check.XXXXXX";
    if (!mkdtemp(tmpl)) { perror("mkdtemp"); return 2; }
    const std::string top = tmpl;
    check_sha256();
    check_round_trip(top);
    check_damage(top);
    check_directories(top);
    check_seal_in_place(top);
    check_cache_dir();
    // the scratch directory goes away again (this program made everything in it)
    if (nftw(top.c_str(), [](const char *p, const struct stat *, int, struct FTW *) { return remove(p); }, 16, FTW_DEPTH | FTW_PHYS) != 0)
        fprintf(stderr, "codecache_check: could not remove %s\n", top.c_str());
    if (g_failed) { fprintf(stderr, "codecache_check: %d checks failed\n", g_failed); return 1; }
    printf("codecache_check ok\n");
    return 0;
}
