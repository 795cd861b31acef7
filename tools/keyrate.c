// keyrate.c -- host rate of the parameter key functions of a built libsentinel_gpu.so (exact
// parameter keys): a loop of sg_param_key, and -- where the library has it -- sg_param_intern_batch on a fresh
// engine, over 1M distinct Strings (inserts, then hits) and 1M repeats of 1,000 of them.  One JSON line a run.
//
//   gcc -O2 -o keyrate tools/keyrate.c -ldl && ./keyrate sentinel_amd/libsentinel_gpu.so
// (a library of an earlier commit gives the sg_param_key baseline; the intern part needs a GPU)
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "../include/sentinel_gpu.h"
static double now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + t.tv_nsec * 1e-9; }
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    void* h = dlopen(argv[1], RTLD_NOW);
    if (!h) { printf("dlopen: %s\n", dlerror()); return 1; }
    int (*key)(sg_engine*, const char*, const char*, uint64_t*) = dlsym(h, "sg_param_key");
    int (*batch)(sg_engine*, const char* const*, const char* const*, uint32_t, uint64_t*) = dlsym(h, "sg_param_intern_batch");
    const uint32_t N = 1000000;
    char** s = malloc(N * sizeof(char*));
    const char** rep = malloc(N * sizeof(char*));
    const char** ty = malloc(N * sizeof(char*));
    uint64_t* out = malloc(N * 8);
    for (uint32_t i = 0; i < N; ++i) { s[i] = malloc(40); snprintf(s[i], 40, "user-%07u-session-token", i * 2654435761u % 10000000u + i); ty[i] = "java.lang.String"; }
    for (uint32_t i = 0; i < N; ++i) rep[i] = s[(i * 2654435761u) % 1000u];
    uint64_t acc = 0;
    for (int r = 0; r < 3; ++r) {
        double t0 = now();
        for (uint32_t i = 0; i < N; ++i) { key(NULL, s[i], ty[i], &out[i]); acc ^= out[i]; }
        double t1 = now();
        for (uint32_t i = 0; i < N; ++i) { key(NULL, rep[i], ty[i], &out[i]); acc ^= out[i]; }
        double t2 = now();
        printf("{\"lib\": \"%s\", \"what\": \"sg_param_key loop\", \"run\": %d, \"distinct_1M_Mkeys_s\": %.2f, \"repeats_of_1000_Mkeys_s\": %.2f}\n", argv[1], r, N / (t1 - t0) / 1e6, N / (t2 - t1) / 1e6);
    }
    if (batch) {
        void (*cfgd)(sg_config*) = dlsym(h, "sg_config_default");
        int (*create)(const sg_config*, sg_engine**) = dlsym(h, "sg_engine_create");
        int (*destroy)(sg_engine*) = dlsym(h, "sg_engine_destroy");
        for (int r = 0; r < 3; ++r) {
            sg_config c; cfgd(&c); c.max_resources = 1024; c.status_ring_log2 = 20;
            sg_engine* e = NULL;
            if (create(&c, &e)) { printf("engine create failed\n"); return 1; }
            double t0 = now();
            batch(e, (const char* const*)s, ty, N, out);
            double t1 = now();
            batch(e, (const char* const*)s, ty, N, out);
            double t2 = now();
            batch(e, rep, ty, N, out);
            double t3 = now();
            printf("{\"lib\": \"%s\", \"what\": \"sg_param_intern_batch\", \"run\": %d, \"distinct_1M_insert_Mkeys_s\": %.2f, \"distinct_1M_hit_Mkeys_s\": %.2f, \"repeats_of_1000_Mkeys_s\": %.2f}\n", argv[1], r, N / (t1 - t0) / 1e6, N / (t2 - t1) / 1e6, N / (t3 - t2) / 1e6);
            destroy(e);
        }
    }
    printf("# %llx\n", (unsigned long long)acc);
    return 0;
}
