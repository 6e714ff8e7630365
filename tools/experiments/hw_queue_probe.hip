// How does the HIP runtime map streams to hardware queues when GPU_MAX_HW_QUEUES is small?  A proof pool opens far more streams than
// four queues; a short kernel whose stream shares a hardware queue with a stream that runs a long kernel starts when the long one ends.
// One long kernel (~100 ms, one workgroup: it leaves the chip empty, so only the QUEUE can hold a short kernel back) on one stream, one
// short kernel on each of the other streams, all enqueued at once; per short kernel, the time from the long kernel's start to its end.
// "held" = it ended after 60 % of the long kernel.  Streams are created in the pool's order: default-class streams first (s0 .. s11),
// then one stream of the lowest and one of the highest priority.  Cases:
//   long on s0 (created first), on s5, on s11 (created last); long on the lowest / highest class; FOUR long kernels on s0 .. s3 (what four
//   per-commitment lane launches of a group do); long on the lowest class with the shorts on twelve default streams AND the highest one.
// hipcc --offload-arch=gfx950 -O2 -o build/hw_queue_probe tools/experiments/hw_queue_probe.hip ;  usage: hw_queue_probe   (reads nothing)
// The iteration counts bound every kernel: nothing here waits on memory or on another kernel.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

__global__ void spin_kernel(unsigned long long* out, unsigned iters) {
    unsigned long long a = threadIdx.x;
    for (unsigned i = 0; i < iters; i++) a = a * 6364136223846793005ull + 1442695040888963407ull;
    if (a == 42) out[0] = a;
}

#define CHECK(x)                                                                              \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) {                                                               \
            printf("%s failed: %s\n", #x, hipGetErrorString(e_));                             \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

static const int N_DEF = 12, N_ALL = N_DEF + 2;  // s0 .. s11 default class, [12] lowest, [13] highest
static const unsigned LONG_ITERS = 3500000, SHORT_ITERS = 350;

static hipStream_t st[N_ALL];
static hipEvent_t t0[N_ALL], t1[N_ALL];
static unsigned long long* d;

static const char* name_of(int i) {
    static char buf[N_ALL][8];
    if (i == N_DEF) return "low";
    if (i == N_DEF + 1) return "high";
    snprintf(buf[i], sizeof buf[i], "s%d", i);
    return buf[i];
}

// long kernels on the streams of `longs`, a short kernel on every other stream below `n_short_limit`
static int run_case(const char* what, const int* longs, int n_long, bool with_prio_shorts) {
    bool is_long[N_ALL] = {};
    for (int k = 0; k < n_long; k++) is_long[longs[k]] = true;
    for (int k = 0; k < n_long; k++) {
        CHECK(hipEventRecord(t0[longs[k]], st[longs[k]]));
        spin_kernel<<<1, 64, 0, st[longs[k]]>>>(d, LONG_ITERS);
        CHECK(hipEventRecord(t1[longs[k]], st[longs[k]]));
    }
    const int n = with_prio_shorts ? N_ALL : N_DEF;
    for (int i = 0; i < n; i++) {
        if (is_long[i]) continue;
        CHECK(hipEventRecord(t0[i], st[i]));
        spin_kernel<<<1, 64, 0, st[i]>>>(d, SHORT_ITERS);
        CHECK(hipEventRecord(t1[i], st[i]));
    }
    CHECK(hipDeviceSynchronize());
    float long_ms = 0;
    CHECK(hipEventElapsedTime(&long_ms, t0[longs[0]], t1[longs[0]]));
    printf("%s: long kernel %.1f ms;", what, long_ms);
    int held = 0, shorts = 0;
    for (int i = 0; i < n; i++) {
        if (is_long[i]) continue;
        float end_ms = 0;
        CHECK(hipEventElapsedTime(&end_ms, t0[longs[0]], t1[i]));
        shorts++;
        const bool h = end_ms > 0.6f * long_ms;
        held += h;
        printf(" %s %.1f%s", name_of(i), end_ms, h ? "*" : "");
    }
    printf("  -> %d of %d short kernels held (*) behind a long one\n", held, shorts);
    return 0;
}

int main() {
    const char* env = getenv("GPU_MAX_HW_QUEUES");
    printf("GPU_MAX_HW_QUEUES=%s\n", env ? env : "(unset: HIP's default, 4)");
    CHECK(hipMalloc(&d, 4096));
    int least = 0, greatest = 0;
    CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    printf("stream priority range: lowest %d, highest %d\n", least, greatest);
    for (int i = 0; i < N_DEF; i++) CHECK(hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking));
    CHECK(hipStreamCreateWithPriority(&st[N_DEF], hipStreamNonBlocking, least));
    CHECK(hipStreamCreateWithPriority(&st[N_DEF + 1], hipStreamNonBlocking, greatest));
    for (int i = 0; i < N_ALL; i++) {
        CHECK(hipEventCreate(&t0[i]));
        CHECK(hipEventCreate(&t1[i]));
        spin_kernel<<<1, 64, 0, st[i]>>>(d, SHORT_ITERS);  // every stream has been used once, in creation order
    }
    CHECK(hipDeviceSynchronize());
    const int first[] = {0}, mid[] = {5}, last[] = {11}, low[] = {N_DEF}, high[] = {N_DEF + 1}, four[] = {0, 1, 2, 3}, two[] = {0, 1};
    if (run_case("long on s0 (created first)", first, 1, false)) return 1;
    if (run_case("long on s5", mid, 1, false)) return 1;
    if (run_case("long on s11 (created last)", last, 1, false)) return 1;
    if (run_case("long on the lowest-priority stream", low, 1, false)) return 1;
    if (run_case("long on the highest-priority stream", high, 1, false)) return 1;
    if (run_case("four long kernels on s0..s3", four, 4, false)) return 1;
    if (run_case("two long kernels on s0, s1", two, 2, false)) return 1;
    if (run_case("long on the lowest-priority stream, shorts on every other stream", low, 1, true)) return 1;
    return 0;
}
