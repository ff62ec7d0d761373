// packet_cost.hip — what one stream operation between two kernels costs on this GPU, and what dispatch-bound events report.
//   hipcc -O2 --offload-arch=gfx950 -o packet_cost packet_cost.hip && ./packet_cost [repetitions]
// Two tiny kernels (one wave each) note the device's wall clock when they start and when they end; the first one idles for 60 us so that the host
// has queued everything behind it long before it ends.  The "gap" is start(second) - end(first), median and minimum over the repetitions; the
// first line (nothing in between) is the floor every other line is read against.  Part 2 hands over between two streams the three ways the
// encoder could; part 3 compares hipEventElapsedTime of events bound to dispatches (hipExtLaunchKernelGGL) with the kernels' own clocks.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(1); } } while (0)

__global__ void tick_kernel(unsigned long long* out, unsigned long long idleTicks) {
    const unsigned long long t0 = wall_clock64();
    unsigned long long t1 = t0;
    for (int i = 0; i < (1 << 22) && t1 - t0 < idleTicks; i++) t1 = wall_clock64();   // bounded: ends by itself whatever the clock does
    if (threadIdx.x == 0) { out[0] = t0; out[1] = wall_clock64(); }
}

static double g_usPerTick = 0.01;
static unsigned long long* g_dev = nullptr;          // [0..1] first kernel, [2..3] second kernel
static unsigned long long g_host[4];

struct Stat { std::vector<double> v; void add(double x) { v.push_back(x); } double med() { std::sort(v.begin(), v.end()); return v[v.size() / 2]; } double mn() { return *std::min_element(v.begin(), v.end()); } };

static double fetch_gap(hipStream_t a, hipStream_t b) {
    CK(hipStreamSynchronize(a)); if (b) CK(hipStreamSynchronize(b));
    CK(hipMemcpy(g_host, g_dev, sizeof g_host, hipMemcpyDeviceToHost));
    return ((double)g_host[2] - (double)g_host[1]) * g_usPerTick;
}

int main(int argc, char** argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 200;
    int rateKHz = 0;
    CK(hipSetDevice(0));
    CK(hipDeviceGetAttribute(&rateKHz, hipDeviceAttributeWallClockRate, 0));
    if (rateKHz > 0) g_usPerTick = 1e3 / rateKHz;
    const unsigned long long idle = (unsigned long long)(60.0 / g_usPerTick), brief = (unsigned long long)(2.0 / g_usPerTick);
    CK(hipMalloc(&g_dev, sizeof g_host));
    hipStream_t s1, s2, aux;
    CK(hipStreamCreateWithFlags(&s1, hipStreamNonBlocking)); CK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking)); CK(hipStreamCreateWithFlags(&aux, hipStreamNonBlocking));
    hipEvent_t timed, timed2, plain, plain2, done, kev[4];
    CK(hipEventCreate(&timed)); CK(hipEventCreate(&timed2)); CK(hipEventCreateWithFlags(&plain, hipEventDisableTiming)); CK(hipEventCreateWithFlags(&plain2, hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    for (auto& e : kev) CK(hipEventCreate(&e));
    printf("wall clock %d kHz, %d repetitions; gap = start of the second kernel - end of the first, us (median / min)\n", rateKHz, reps);

    // ---- part 1: one operation between two kernels of one stream ----
    const char* names[] = { "nothing (floor)", "timed hipEventRecord", "hipEventDisableTiming record", "same-stream no-op (wait on an event of this stream)",
                            "cross-stream wait, event already complete", "event pair bound to the 2nd dispatch (hipExtLaunchKernelGGL)",
                            "event pairs bound to both dispatches" };
    for (int op = 0; op < 7; op++) {
        Stat st;
        for (int r = 0; r < reps + 3; r++) {
            if (op == 4) { CK(hipEventRecord(done, s2)); CK(hipEventSynchronize(done)); }
            if (op == 6) hipExtLaunchKernelGGL(tick_kernel, dim3(1), dim3(64), 0, s1, kev[0], kev[1], 0, g_dev, idle);
            else hipLaunchKernelGGL(tick_kernel, dim3(1), dim3(64), 0, s1, g_dev, idle);
            if (op == 1) CK(hipEventRecord(timed, s1));
            if (op == 2) CK(hipEventRecord(plain, s1));
            if (op == 3) { CK(hipEventRecord(plain, s1)); CK(hipStreamWaitEvent(s1, plain, 0)); }
            if (op == 4) CK(hipStreamWaitEvent(s1, done, 0));
            if (op == 5 || op == 6) hipExtLaunchKernelGGL(tick_kernel, dim3(1), dim3(64), 0, s1, kev[2], kev[3], 0, g_dev + 2, brief);
            else hipLaunchKernelGGL(tick_kernel, dim3(1), dim3(64), 0, s1, g_dev + 2, brief);
            CK(hipGetLastError());
            const double g = fetch_gap(s1, nullptr);
            if (r >= 3) st.add(g);
        }
        printf("op %d  %-62s %7.2f / %7.2f\n", op, names[op], st.med(), st.mn());
    }
    printf("(op 3 holds a record and the wait; its cost over op 2 is the wait's)\n");

    // ---- part 2: the first kernel on stream 1, the second on stream 2, ordered behind it ----
    const char* hnames[] = { "wait on the stop event bound to the 1st dispatch",
                             "record (no timing) behind the 1st kernel, wait on it",
                             "timed record behind the 1st kernel, wait on it",
                             "timed record, wait, then a timed record in front of the 2nd kernel (direct wait, parent's timing records)",
                             "timed record; wait + record on a third stream; wait on that; timed record (the parent's relay)" };
    for (int h = 0; h < 5; h++) {
        Stat st; int disorder = 0;
        for (int r = 0; r < reps + 3; r++) {
            if (h == 0) hipExtLaunchKernelGGL(tick_kernel, dim3(1), dim3(64), 0, s1, kev[0], kev[1], 0, g_dev, idle);
            else hipLaunchKernelGGL(tick_kernel, dim3(1), dim3(64), 0, s1, g_dev, idle);
            hipEvent_t w = h == 0 ? kev[1] : h == 1 ? plain : timed;
            if (h >= 1) CK(hipEventRecord(w, s1));
            if (h == 4) { CK(hipStreamWaitEvent(aux, w, 0)); CK(hipEventRecord(plain2, aux)); w = plain2; }
            CK(hipStreamWaitEvent(s2, w, 0));
            if (h >= 3) CK(hipEventRecord(timed2, s2));
            hipLaunchKernelGGL(tick_kernel, dim3(1), dim3(64), 0, s2, g_dev + 2, brief);
            CK(hipGetLastError());
            CK(hipStreamSynchronize(aux));
            const double g = fetch_gap(s1, s2);
            if (g < 0) disorder++;
            if (r >= 3) st.add(g);
        }
        printf("handover %d  %-104s %7.2f / %7.2f   out of order: %d\n", h, hnames[h], st.med(), st.mn(), disorder);
    }

    // ---- part 3: what events bound to dispatches report ----
    {
        Stat dk, de, gk, ge, sk, se; int errs = 0;
        for (int r = 0; r < reps + 3; r++) {
            hipExtLaunchKernelGGL(tick_kernel, dim3(1), dim3(64), 0, s1, kev[0], kev[1], 0, g_dev, idle);
            hipExtLaunchKernelGGL(tick_kernel, dim3(1), dim3(64), 0, s1, kev[2], kev[3], 0, g_dev + 2, brief);
            CK(hipGetLastError());
            const double g = fetch_gap(s1, nullptr);
            float a = -1, b = -1, c = -1;
            if (hipEventElapsedTime(&a, kev[0], kev[1]) != hipSuccess || hipEventElapsedTime(&b, kev[1], kev[2]) != hipSuccess || hipEventElapsedTime(&c, kev[0], kev[3]) != hipSuccess) { errs++; (void)hipGetLastError(); continue; }
            if (r < 3) continue;
            dk.add((g_host[1] - g_host[0]) * g_usPerTick); de.add(a * 1e3);
            gk.add(g); ge.add(b * 1e3);
            sk.add((g_host[3] - g_host[0]) * g_usPerTick); se.add(c * 1e3);
        }
        printf("bound events, %d hipEventElapsedTime errors; us, median: kernel clock against hipEventElapsedTime\n", errs);
        if (!dk.v.empty()) {
            printf("  first kernel, its own start -> stop event            %8.2f  %8.2f\n", dk.med(), de.med());
            printf("  stop of the first -> start of the second (gap)       %8.2f  %8.2f\n", gk.med(), ge.med());
            printf("  start of the first -> stop of the second (span)      %8.2f  %8.2f\n", sk.med(), se.med());
        }
        // a pair that is bound again while its first dispatch is still pending (ring reuse): the second binding must win and nothing may fail
        hipExtLaunchKernelGGL(tick_kernel, dim3(1), dim3(64), 0, s1, kev[0], kev[1], 0, g_dev, idle);
        hipExtLaunchKernelGGL(tick_kernel, dim3(1), dim3(64), 0, s1, kev[0], kev[1], 0, g_dev + 2, brief);
        CK(hipGetLastError());
        CK(hipEventSynchronize(kev[1]));
        const hipError_t q = hipStreamQuery(s1);
        float a = -1; const hipError_t e = hipEventElapsedTime(&a, kev[0], kev[1]);
        CK(hipStreamSynchronize(s1));
        printf("  pair bound twice, first dispatch pending: stream %s after hipEventSynchronize(stop); elapsed %s %.2f us (the second kernel idles 2 us, the first 60)\n",
               q == hipSuccess ? "idle" : "still busy", e == hipSuccess ? "ok" : hipGetErrorString(e), a * 1e3);
        (void)hipGetLastError();
        // an event that was never bound or recorded next to one that was
        hipEvent_t fresh; CK(hipEventCreate(&fresh));
        const hipError_t e2 = hipEventElapsedTime(&a, fresh, kev[1]);
        printf("  elapsed(never recorded, bound): %s\n", e2 == hipSuccess ? "ok" : hipGetErrorString(e2));
        (void)hipGetLastError();
        // mixed: a stand-alone timed record behind a kernel with bound events
        hipExtLaunchKernelGGL(tick_kernel, dim3(1), dim3(64), 0, s1, kev[0], kev[1], 0, g_dev, brief);
        CK(hipEventRecord(timed, s1));
        CK(hipStreamSynchronize(s1));
        const hipError_t e3 = hipEventElapsedTime(&a, kev[0], timed);
        printf("  elapsed(bound start, stand-alone record behind the kernel): %s %.2f us\n", e3 == hipSuccess ? "ok" : hipGetErrorString(e3), a * 1e3);
        (void)hipGetLastError();
        CK(hipEventDestroy(fresh));
    }
    CK(hipDeviceSynchronize());
    return 0;
}
