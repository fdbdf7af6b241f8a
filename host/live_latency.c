/*
 * host/live_latency.c — wall time of every Spleeter4StemsProcessSamples call of the LIVE mode (Spleeter4StemsInitLive), as the plugin's
 * audio callback sees it.
 *
 *     live_latency F T hops_per_run lookahead hops weights.f32 pace_us out.json [instances [sample_rate [call_size]]]
 *
 * Same measurement as host/rt_latency.c (the plugin mode): `instances` independent objects on as many host threads, one hop (1024
 * samples) per call, `hops` calls each, clock_gettime around every call; pace_us = 0 calls back to back, 23220 once per real-time hop
 * period.  In the live mode a network run is started every hops_per_run hops and joined hops_per_run hops later, so there is no
 * separate class of join hops: the JSON reports p50 / p99 / max over all calls, the instance's Spleeter4StemsLatency and its output peak.
 * With sample_rate the instances are rate instances (Spleeter4StemsInitRate, maxBlock = call_size) and `hops` counts calls of call_size samples
 * (default 1024) at that rate; pace_us is then the caller's block period.
 * weights.f32 holds 4 spleeterCoeff blobs (drum, bass, accompaniment, vocal).  Plain C against include/Spleeter4Stems.h; used by
 * tests/test_live.py and scripts/live_bench.py.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "Spleeter4Stems.h"
#include "spleeterrt_amd.h"      /* srtLastError(): why an instance came up muted, if it did */

#define COEFF_BYTES 39290900u

static double now_us(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return 1e6 * (double)t.tv_sec + 1e-3 * (double)t.tv_nsec;
}

typedef struct {
    int id, F, T, K, L, hops, pace_us, latency, rate, call;
    void *coeff[4];
    double init_ms, *us;
    float peak;
    char init_error[256];
    pthread_barrier_t *start;
} Job;

static void *run(void *arg)
{
    Job *j = (Job *)arg;
    Spleeter4Stems *msr = (Spleeter4Stems *)malloc(sizeof(Spleeter4Stems));
    const int n = j->call;
    float *inL = (float *)malloc(n * sizeof(float)), *inR = (float *)malloc(n * sizeof(float));
    float *out = (float *)calloc(8 * (size_t)n, sizeof(float)), *ptr[8];
    unsigned lcg = 12345u + 977u * (unsigned)j->id;
    double t0 = now_us();
    if (j->rate) Spleeter4StemsInitRate(msr, j->F, j->T, j->coeff, j->K, j->L, j->rate, n);
    else Spleeter4StemsInitLive(msr, j->F, j->T, j->coeff, j->K, j->L);
    j->init_ms = (now_us() - t0) * 1e-3;
    j->latency = Spleeter4StemsLatency(msr);
    snprintf(j->init_error, sizeof j->init_error, "%s", srtLastError());
    for (char *c = j->init_error; *c; ++c) if (*c == '"' || *c == '\\' || *c < 32) *c = ' ';
    pthread_barrier_wait(j->start);
    double next = now_us();
    for (int h = 0; h < j->hops; ++h) {
        for (int i = 0; i < n; ++i) {
            lcg = lcg * 1664525u + 1013904223u; inL[i] = ((float)(lcg >> 8) / 16777216.0f - 0.5f) * 0.2f;
            lcg = lcg * 1664525u + 1013904223u; inR[i] = ((float)(lcg >> 8) / 16777216.0f - 0.5f) * 0.2f;
        }
        for (int k = 0; k < 8; ++k) ptr[k] = out + n * k;
        if (j->pace_us) {
            next += j->pace_us;
            double w = next - now_us();
            if (w > 0) { struct timespec ts = { (time_t)(w / 1e6), (long)((w - 1e6 * (long)(w / 1e6)) * 1e3) }; nanosleep(&ts, 0); }
        }
        t0 = now_us();
        Spleeter4StemsProcessSamples(msr, inL, inR, n, ptr);
        j->us[h] = now_us() - t0;
        for (int i = 0; i < 8 * n; ++i) { float a = out[i] < 0 ? -out[i] : out[i]; if (a > j->peak) j->peak = a; }
    }
    Spleeter4StemsFree(msr);
    free(msr); free(inL); free(inR); free(out);
    return 0;
}

static int cmp(const void *a, const void *b) { double x = *(const double *)a, y = *(const double *)b; return x < y ? -1 : x > y; }

int main(int argc, char **argv)
{
    if (argc < 9) { fprintf(stderr, "usage: %s F T hops_per_run lookahead hops weights.f32 pace_us out.json [instances [sample_rate [call_size]]]\n", argv[0]); return 2; }
    const int F = atoi(argv[1]), T = atoi(argv[2]), K = atoi(argv[3]), L = atoi(argv[4]), hops = atoi(argv[5]), pace = atoi(argv[7]);
    const int ni = argc > 9 ? atoi(argv[9]) : 2, rate = argc > 10 ? atoi(argv[10]) : 0, call = argc > 11 ? atoi(argv[11]) : 1024;
    if (F < 64 || T < 64 || K < 1 || K > T || L < 0 || L > T - K || hops < 1 || ni < 1 || ni > 16 || rate < 0 || call < 1 || call > 65536 || (!rate && call != 1024)) { fprintf(stderr, "bad arguments\n"); return 2; }
    FILE *wf = fopen(argv[6], "rb");
    char *blob = (char *)malloc((size_t)4 * COEFF_BYTES);
    if (!wf || !blob || fread(blob, COEFF_BYTES, 4, wf) != 4) { fprintf(stderr, "cannot read 4 coefficient blobs from %s\n", argv[6]); return 1; }
    fclose(wf);
    pthread_barrier_t start;
    pthread_barrier_init(&start, 0, (unsigned)ni);
    Job *jobs = (Job *)calloc((size_t)ni, sizeof(Job));
    pthread_t *th = (pthread_t *)calloc((size_t)ni, sizeof(pthread_t));
    for (int i = 0; i < ni; ++i) {
        Job *j = &jobs[i];
        j->id = i; j->F = F; j->T = T; j->K = K; j->L = L; j->hops = hops; j->pace_us = pace; j->start = &start; j->rate = rate; j->call = call;
        for (int k = 0; k < 4; ++k) j->coeff[k] = blob + (size_t)k * COEFF_BYTES;
        j->us = (double *)calloc((size_t)hops, sizeof(double));
        pthread_create(&th[i], 0, run, j);
    }
    for (int i = 0; i < ni; ++i) pthread_join(th[i], 0);
    FILE *f = fopen(argv[8], "w");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[8]); return 1; }
    fprintf(f, "{\"F\": %d, \"T\": %d, \"hops_per_run\": %d, \"lookahead\": %d, \"hops\": %d, \"pace_us\": %d, \"sample_rate\": %d, \"call_size\": %d, \"instances\": [", F, T, K, L, hops, pace, rate ? rate : 44100, call);
    for (int i = 0; i < ni; ++i) {
        Job *j = &jobs[i];
        int worst = 0;
        for (int h = 1; h < hops; ++h) if (j->us[h] > j->us[worst]) worst = h;
        qsort(j->us, (size_t)hops, sizeof(double), cmp);
        const int i99 = (int)(0.99 * (hops - 1) + 0.5);
        fprintf(f, "%s{\"init_ms\": %.1f, \"init_error\": \"%s\", \"latency_samples\": %d, \"output_peak\": %.6g, \"worst_hop\": %d, "
                   "\"calls\": {\"n\": %d, \"p50_us\": %.1f, \"p99_us\": %.1f, \"max_us\": %.1f}}",
                i ? ", " : "", j->init_ms, j->init_error, j->latency, j->peak, worst, hops, j->us[hops / 2], j->us[i99], j->us[hops - 1]);
    }
    fprintf(f, "]}\n");
    fclose(f);
    return 0;
}
