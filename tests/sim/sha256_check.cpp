// sha256_check.cpp -- the host SHA-256 of dcdf_amd/csrc/k2r_sha256_host.h against digests computed elsewhere (hashlib), as a
// stand-alone program: built with AddressSanitizer and UBSan by tests/test_sha256_host.py, nothing of it is loaded into Python.
//
//   sha256_check CASES
//
// CASES holds one message per line:  <offset> <length> <digest, 64 hex digits> <message, 2 * length hex digits or "-">.
// Every message is copied to the END of an allocation of exactly offset + length bytes, so that it starts `offset` bytes into the
// allocation and a read past its last byte is a read past the allocation.  For every message:
//   host      sha256_host (padding + the dispatching block function) gives the digest;
//   portable  blocks_portable over the message padded HERE (0x80, zeros, the bit count) gives the digest;
//   shani     blocks_shani likewise, when the CPU has the extension.
// Then, for random starting states and 0..5 blocks of random data at every misalignment 0..7, blocks_portable, the dispatching
// blocks and (when present) blocks_shani must leave identical states.
//
// Output: "impl <name> ran|absent" per implementation, "dispatch <name>", one "MISMATCH <check> len=<n> offset=<o> ..." line per
// failure, "messages <n>" and "states <n>".  Exit status 0 when every check RAN (mismatches are in the output), 2 on bad input.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../dcdf_amd/csrc/k2r_sha256_host.h"

namespace sd = k2r::sha256_detail;
typedef void (*BlockFn)(uint32_t*, const uint8_t*, size_t);

static const uint32_t kInit[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};

static int hexval(char c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    return -1;
}

static bool unhex(const std::string& s, uint8_t* out, size_t n) {
    if (s.size() != 2 * n) return false;
    for (size_t i = 0; i < n; i++) {
        const int a = hexval(s[2 * i]), b = hexval(s[2 * i + 1]);
        if (a < 0 || b < 0) return false;
        out[i] = (uint8_t)(a * 16 + b);
    }
    return true;
}

static std::string hex(const uint8_t* p, size_t n) {
    static const char d[] = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) {
        s += d[p[i] >> 4];
        s += d[p[i] & 15];
    }
    return s;
}

// the digest of msg[0..len) by `fn`, the padding written out here: msg | 0x80 | zeros | bit count (big-endian, 8 bytes)
static void digest_by(BlockFn fn, const uint8_t* msg, size_t len, uint8_t out[32]) {
    const size_t padded = (len + 1 + 8 + 63) / 64 * 64;
    std::vector<uint8_t> m(padded, 0);
    if (len) memcpy(m.data(), msg, len);
    m[len] = 0x80;
    const uint64_t bits = (uint64_t)len * 8;
    for (int i = 0; i < 8; i++) m[padded - 1 - i] = (uint8_t)(bits >> (8 * i));
    uint32_t st[8];
    memcpy(st, kInit, sizeof(st));
    fn(st, m.data(), padded / 64);
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 4; j++) out[4 * i + j] = (uint8_t)(st[i] >> (24 - 8 * j));
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: sha256_check CASES\n");
        return 2;
    }
    bool shani = false;
#if defined(__x86_64__)
    shani = sd::have_shani();
#endif
    printf("impl portable ran\n");
    printf("impl shani %s\n", shani ? "ran" : "absent");
    printf("dispatch %s\n", shani ? "shani" : "portable");

    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    size_t messages = 0;
    std::string sdig, smsg;
    size_t off, len;
    while (in >> off >> len >> sdig >> smsg) {
        uint8_t want[32], got[32];
        uint8_t* buf = new uint8_t[off + len];  // the message ends where the allocation ends
        if (!unhex(sdig, want, 32) || !(len == 0 ? smsg == "-" : unhex(smsg, buf + off, len))) {
            fprintf(stderr, "bad case line %zu\n", messages + 1);
            return 2;
        }
        const uint8_t* msg = buf + off;
        k2r::sha256_host(msg, len, got);
        if (memcmp(got, want, 32)) printf("MISMATCH host len=%zu offset=%zu got=%s want=%s\n", len, off, hex(got, 32).c_str(), sdig.c_str());
        digest_by(sd::blocks_portable, msg, len, got);
        if (memcmp(got, want, 32)) printf("MISMATCH portable len=%zu offset=%zu got=%s want=%s\n", len, off, hex(got, 32).c_str(), sdig.c_str());
#if defined(__x86_64__)
        if (shani) {
            digest_by(sd::blocks_shani, msg, len, got);
            if (memcmp(got, want, 32)) printf("MISMATCH shani len=%zu offset=%zu got=%s want=%s\n", len, off, hex(got, 32).c_str(), sdig.c_str());
        }
#endif
        delete[] buf;
        messages++;
    }
    if (!in.eof()) {
        fprintf(stderr, "bad case line %zu\n", messages + 1);
        return 2;
    }
    printf("messages %zu\n", messages);

    // the block functions on the same state and data: random starting states, 0..5 blocks, every misalignment of the data
    size_t states = 0;
    for (int trial = 0; trial < 50; trial++)
        for (size_t nb = 0; nb <= 5; nb++) {
            const size_t mis = (size_t)(trial % 8), n = 64 * nb;
            uint8_t* buf = new uint8_t[mis + n];
            for (size_t i = 0; i < mis + n; i++) buf[i] = (uint8_t)rnd();
            uint32_t st0[8], a[8], b[8];
            for (int i = 0; i < 8; i++) st0[i] = (uint32_t)rnd();
            memcpy(a, st0, sizeof(a));
            memcpy(b, st0, sizeof(b));
            sd::blocks_portable(a, buf + mis, nb);
            sd::blocks(b, buf + mis, nb);
            if (memcmp(a, b, sizeof(a))) printf("MISMATCH state-dispatch len=%zu offset=%zu trial=%d\n", n, mis, trial);
            if (nb == 0 && memcmp(a, st0, sizeof(a))) printf("MISMATCH state-zero-blocks len=0 offset=%zu trial=%d\n", mis, trial);
#if defined(__x86_64__)
            if (shani) {
                memcpy(b, st0, sizeof(b));
                sd::blocks_shani(b, buf + mis, nb);
                if (memcmp(a, b, sizeof(a))) printf("MISMATCH state-shani len=%zu offset=%zu trial=%d\n", n, mis, trial);
            }
#endif
            delete[] buf;
            states++;
        }
    printf("states %zu\n", states);
    return 0;
}
