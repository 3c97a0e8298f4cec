/*
 * album_mock.c -- a broker stand-in for tests/test_broker_album_host.py (compiled by that test): creates the segment and
 * answers every request with the request's own input, in place -- out_offset 0, out_bytes = in_bytes -- and with the GIF
 * fields of the slot echoed in the answer's geometry (out_w = in_pages, out_h = in_page, out_c = in_destructive,
 * out_step = in_kind), so the test reads back exactly what glue/imp_gpu_client.c wrote for an IMPB_IN_GIF request.
 *   album_mock <name> <slots> <slot_kb>       "ready" on stdout once the segment is served; SIGTERM stops it
 */
#define _GNU_SOURCE
#include <impgpu_broker.h>
#include <fcntl.h>
#include <linux/futex.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <time.h>
#include <unistd.h>

static volatile sig_atomic_t g_stop;
static void on_term(int s) { (void)s; g_stop = 1; }

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s name slots slot_kb\n", argv[0]); return 2; }
    const char* name = argv[1];
    const int nslots = atoi(argv[2]);
    const uint64_t slot_bytes = (uint64_t)atoi(argv[3]) << 10;
    const uint64_t slots_offset = sizeof(impb_header), data_offset = slots_offset + (uint64_t)nslots * sizeof(impb_slot);
    const uint64_t total = data_offset + (uint64_t)nslots * slot_bytes;
    struct sigaction sa;
    memset(&sa, 0, sizeof sa);
    sa.sa_handler = on_term;
    sigaction(SIGTERM, &sa, NULL);
    shm_unlink(name);
    int fd = shm_open(name, O_RDWR | O_CREAT | O_EXCL, 0600);
    if (fd < 0 || ftruncate(fd, (off_t)total) != 0) { perror("shm"); return 3; }
    uint8_t* base = (uint8_t*)mmap(NULL, total, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (base == MAP_FAILED) { perror("mmap"); return 3; }
    impb_header_fields* h = &((impb_header*)base)->f;
    impb_slot* slots = (impb_slot*)(base + slots_offset);
    h->magic = IMPB_MAGIC; h->version = IMPB_VERSION; h->nslots = (uint32_t)nslots;
    h->slot_data_bytes = slot_bytes; h->slots_offset = slots_offset; h->data_offset = data_offset;
    h->epoch = 1;
    __atomic_store_n(&h->broker_pid, (uint32_t)getpid(), __ATOMIC_RELEASE);
    printf("ready\n");
    fflush(stdout);
    while (!g_stop) {
        int served = 0;
        for (int i = 0; i < nslots; i++) {
            impb_slot_fields* s = &slots[i].f;
            uint32_t expect = IMPB_SUBMITTED;
            if (!__atomic_compare_exchange_n(&s->state, &expect, (uint32_t)IMPB_TAKEN, 0, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED)) continue;
            s->code = IMP_OK; s->step = IMP_STEP_ENCODE;
            s->out_offset = 0; s->out_bytes = s->in_bytes <= slot_bytes ? s->in_bytes : 0;
            s->out_w = s->in_pages; s->out_h = s->in_page; s->out_c = s->in_destructive; s->out_step = (int32_t)s->in_kind;
            s->out_frames = 1; s->out_frame_stride = s->out_bytes;
            s->batch_size = 1; s->error[0] = 0;
            __atomic_add_fetch(&h->served, (uint64_t)1, __ATOMIC_RELAXED);
            __atomic_store_n(&s->state, (uint32_t)IMPB_DONE, __ATOMIC_RELEASE);
            syscall(SYS_futex, &s->state, FUTEX_WAKE, 1, NULL, NULL, 0);
            served++;
        }
        if (!served) {
            struct timespec nap = {0, 200 * 1000};
            nanosleep(&nap, NULL);
        }
    }
    __atomic_store_n(&h->broker_pid, 0u, __ATOMIC_RELEASE);
    munmap(base, total);
    shm_unlink(name);
    return 0;
}
