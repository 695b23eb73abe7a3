// Driver of the CPU build of the engine (tests/test_engine_cpu_host.py): csrc/engine.hip compiled as host C++ against
// the HIP stand-in of tests/native/hipcpu, linked here, and driven through its C ABI by a call list that Python wrote.
//
//   engine_cpu_driver LIST OUT
//
// LIST: "SGCL", then calls to the end of the file (a pipe will do: every call's output is flushed before the next call
//   is read); per call u16 name length, name, u32 args; per argument one kind byte and
//   0 value    i64 (an integer, or a raw pointer value such as NULL)
//   1 buffer   u64 bytes, the bytes: copied into a malloc block of exactly that size (so that a sanitizer sees the
//              engine leave a host buffer too), passed as a pointer, written to OUT after the call
//   2 null
//   3 handle   u32 id: the ctx or circuit an earlier call stored under that id
//   4 handle*  u32 id: a pointer to the slot of that id (sgfhe_ctx_create, sgfhe_ctx_clone, sgfhe_circuit_create*)
//   5 device   u64 bytes, the bytes: as kind 1, but in memory of hipMalloc (the *_device entries)
// OUT: "SGCO"; per call i64 result, u32 text length, text (the string an entry returned, or
//   sgfhe_last_error_string of the call's ctx after a status other than 0), then per buffer argument u64 bytes, the bytes.
// Everything is little-endian.  Nothing here knows a parameter set or a shape: they are in the list.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/sgfhe_hip.h"

namespace {

struct Arg {
    int kind = 0;
    int64_t val = 0;
    void *ptr = nullptr;
    uint64_t bytes = 0;
};
struct Result {
    int64_t value = 0;
    std::string text;
    bool is_status = false;
};

[[noreturn]] void die(const char *what) {
    fprintf(stderr, "engine_cpu_driver: %s\n", what);
    exit(2);
}

template <class T>
T conv(const Arg &a) {
    if constexpr (std::is_pointer<T>::value) return reinterpret_cast<T>(a.ptr);
    else return static_cast<T>(a.val);
}
template <class R, class... A, size_t... I>
Result invoke(R (*f)(A...), const std::vector<Arg> &v, std::index_sequence<I...>) {
    if (v.size() != sizeof...(A)) die("a call with the wrong number of arguments");
    Result r;
    if constexpr (std::is_same<R, const char *>::value) {
        const char *s = f(conv<A>(v[I])...);
        r.text = s ? s : "";
    } else {
        r.value = (int64_t)f(conv<A>(v[I])...);
        r.is_status = std::is_same<R, int>::value;
    }
    return r;
}
template <class R, class... A>
Result call(R (*f)(A...), const std::vector<Arg> &v) { return invoke(f, v, std::index_sequence_for<A...>{}); }

typedef Result (*Entry)(const std::vector<Arg> &);
#define E(name) {#name, [](const std::vector<Arg> &v) { return call(&name, v); }},
const std::map<std::string, Entry> ENTRIES = {
    E(sgfhe_version) E(sgfhe_abi_version) E(sgfhe_build_id) E(sgfhe_ctx_create) E(sgfhe_ctx_create_ex)
    E(sgfhe_ctx_clone) E(sgfhe_set_coalesce) E(sgfhe_coalesce_stats) E(sgfhe_ctx_destroy) E(sgfhe_last_error_string)
    E(sgfhe_set_chunk) E(sgfhe_set_lanes) E(sgfhe_set_small_batch_max) E(sgfhe_set_random_flatten)
    E(sgfhe_set_random_flatten_key) E(sgfhe_bkey_upload) E(sgfhe_bkey_upload_rns2) E(sgfhe_rns2_convert)
    E(sgfhe_bkey_generate) E(sgfhe_bkey_device_form_bytes) E(sgfhe_bkey_export_device_form)
    E(sgfhe_bkey_import_device_form) E(sgfhe_bootstrap_batch) E(sgfhe_bootstrap_batch_device) E(sgfhe_sync)
    E(sgfhe_external_product) E(sgfhe_pack_encrypted_bits) E(sgfhe_debug_cmux) E(sgfhe_debug_accumulators)
    E(sgfhe_debug_digits) E(sgfhe_debug_flatten) E(sgfhe_debug_kloop_step) E(sgfhe_debug_chunk_entry)
    E(sgfhe_debug_chunk_exit) E(sgfhe_debug_ntt) E(sgfhe_debug_primes) E(sgfhe_host_deterministic_expand)
    E(sgfhe_host_encrypt_private) E(sgfhe_host_pack_private) E(sgfhe_host_normalize_private)
    E(sgfhe_host_split_ciphertext) E(sgfhe_host_decrypt_lwe) E(sgfhe_host_decrypt_rlwe) E(sgfhe_host_public_key)
    E(sgfhe_host_encrypt_public) E(sgfhe_host_pack_public) E(sgfhe_host_normalize_public) E(sgfhe_timing_enable)
    E(sgfhe_timing_read) E(sgfhe_kernel_names) E(sgfhe_release_host_staging) E(sgfhe_circuit_create)
    E(sgfhe_circuit_info) E(sgfhe_circuit_destroy) E(sgfhe_circuit_run) E(sgfhe_circuit_run_ct)
    E(sgfhe_circuit_run_ct_ex) E(sgfhe_pack_lwe_modq) E(sgfhe_lwe_noise) E(sgfhe_circuit_run_probe)
    E(sgfhe_circuit_create_lanes) E(sgfhe_circuit_group) E(sgfhe_circuit_create3) E(sgfhe_lwe_lift_modq)
    E(sgfhe_circuit_create_w) E(sgfhe_bootstrap_lut_batch) E(sgfhe_circuit_create_lut)
    E(sgfhe_bootstrap_lut_multi_batch) E(sgfhe_circuit_create_lut_multi) E(sgfhe_circuit_create_data)
    E(sgfhe_circuit_planes) E(sgfhe_circuit_run_data) E(sgfhe_circuit_run_ct_data) E(sgfhe_circuit_run_probe_data)
    E(sgfhe_circuit_create_seq) E(sgfhe_circuit_registers) E(sgfhe_circuit_run_steps) E(sgfhe_circuit_run_steps_ct)
    E(sgfhe_circuit_create_routed) E(sgfhe_circuit_routes) E(sgfhe_circuit_run_device) E(sgfhe_circuit_run_ct_device)
    E(sgfhe_circuit_run_steps_device) E(sgfhe_circuit_run_steps_ct_device) E(sgfhe_debug_circuit_script)
    E(sgfhe_debug_circuit_script_calls)
};
#undef E

FILE *fin, *fout;
void rd(void *p, size_t n) {
    if (n && fread(p, 1, n, fin) != n) die("the call list ends early");
}
void wr(const void *p, size_t n) {
    if (n && fwrite(p, 1, n, fout) != n) die("cannot write the output");
}
template <class T>
T rd() {
    T v;
    rd(&v, sizeof v);
    return v;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) die("usage: engine_cpu_driver LIST OUT");
    fin = fopen(argv[1], "rb");
    fout = fopen(argv[2], "wb");
    if (!fin || !fout) die("cannot open LIST or OUT");
    char magic[4];
    rd(magic, 4);
    if (memcmp(magic, "SGCL", 4)) die("not a call list");
    wr("SGCO", 4);
    fflush(fout);
    std::map<uint32_t, void *> handles;   // id -> ctx or circuit; the slots stay where they are (std::map)
    std::map<uint32_t, bool> is_ctx;
    for (;;) {
        uint16_t nl;
        if (fread(&nl, 1, 2, fin) != 2) break;   // the end of the list
        std::string name(nl, '\0');
        rd(&name[0], nl);
        const auto e = ENTRIES.find(name);
        if (e == ENTRIES.end()) die(("no entry " + name).c_str());
        const uint32_t na = rd<uint32_t>();
        std::vector<Arg> args(na);
        for (Arg &a : args) {
            a.kind = rd<uint8_t>();
            switch (a.kind) {
            case 0:
                a.val = rd<int64_t>();
                a.ptr = reinterpret_cast<void *>((intptr_t)a.val);
                break;
            case 1:
            case 5:
                a.bytes = rd<uint64_t>();
                if (a.kind == 1) a.ptr = malloc(a.bytes ? a.bytes : 1);
                else if (hipMalloc(&a.ptr, a.bytes ? a.bytes : 1) != hipSuccess) die("hipMalloc");
                if (!a.ptr) die("no memory");
                rd(a.ptr, a.bytes);
                break;
            case 2: break;
            case 3: {
                const uint32_t id = rd<uint32_t>();
                if (!handles.count(id)) die("a handle that no call made");
                a.ptr = handles[id];
                a.val = (int64_t)id;
                break;
            }
            case 4: {
                const uint32_t id = rd<uint32_t>();
                handles[id] = nullptr;
                is_ctx[id] = name.compare(0, 10, "sgfhe_ctx_") == 0;
                a.ptr = &handles[id];
                break;
            }
            default: die("an argument of unknown kind");
            }
        }
        Result r = e->second(args);
        if (r.is_status && r.value != 0 && na && args[0].kind == 3 && is_ctx[(uint32_t)args[0].val])
            r.text = sgfhe_last_error_string(static_cast<const sgfhe_ctx *>(args[0].ptr));
        wr(&r.value, 8);
        const uint32_t tl = (uint32_t)r.text.size();
        wr(&tl, 4);
        wr(r.text.data(), tl);
        for (Arg &a : args)
            if (a.kind == 1 || a.kind == 5) {
                wr(&a.bytes, 8);
                wr(a.ptr, a.bytes);
                if (a.kind == 1) free(a.ptr);
                else if (hipFree(a.ptr) != hipSuccess) die("hipFree");
            }
        fflush(fout);
    }
    if (fclose(fout) != 0) die("cannot write the output");
    fclose(fin);
    return 0;
}
