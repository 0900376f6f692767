// az_records.h — the eight per-game record arrays and their packed layout, ONE copy for host and device.
//
// The engine records a generation in eight arrays (n games, mp = max_plies rows per game, mc = max_children per row).  The
// packed layout puts them into one buffer in this order, every array 16-byte aligned (include/az_engine.h,
// az_engine_export_device):
//   game_len i32[n] | game_ret0 f32[n] | states u64[n][mp][2] | move u16[n][mp] | n_children u8[n][mp] |
//   child_action u16[n][mp][mc] | child_visits u32[n][mp][mc] | value f64[n][mp]
// Written by az_engine_export, az_engine_export_device and az_engine_stream_take_device (csrc/az_engine.hip), read by every
// append entry of the replay store (csrc/az_replay.hip); engine.py's device_export_layout is its Python twin.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define AZ_RECORD_ARRAYS 8

struct AzRecords { // one view of the eight arrays (device or host pointers), in the order of the packed layout
    int32_t *game_len;
    float *game_ret0;
    uint64_t *states;
    uint16_t *move;
    uint8_t *n_children;
    uint16_t *child_action;
    uint32_t *child_visits;
    double *value;
};

static inline void records_sizes(size_t n, size_t mp, size_t mc, size_t sizes[AZ_RECORD_ARRAYS]) { // bytes per array
    const size_t s[AZ_RECORD_ARRAYS] = {n * 4, n * 4, n * mp * 16, n * mp * 2, n * mp, n * mp * mc * 2, n * mp * mc * 4, n * mp * 8};
    for (int i = 0; i < AZ_RECORD_ARRAYS; i++) sizes[i] = s[i];
}

static inline void records_offsets(size_t n, size_t mp, size_t mc, size_t off[AZ_RECORD_ARRAYS + 1]) { // off[8] = total bytes
    size_t sizes[AZ_RECORD_ARRAYS];
    records_sizes(n, mp, mc, sizes);
    off[0] = 0;
    for (int i = 0; i < AZ_RECORD_ARRAYS; i++) off[i + 1] = off[i] + ((sizes[i] + 15) & ~(size_t)15);
}

// The arrays of a packed buffer (a reader casts its const buffer once, at the call).
static inline AzRecords records_in(void *buf, size_t n, size_t mp, size_t mc) {
    size_t off[AZ_RECORD_ARRAYS + 1];
    records_offsets(n, mp, mc, off);
    char *b = (char *)buf;
    AzRecords v;
    v.game_len = (int32_t *)(b + off[0]);
    v.game_ret0 = (float *)(b + off[1]);
    v.states = (uint64_t *)(b + off[2]);
    v.move = (uint16_t *)(b + off[3]);
    v.n_children = (uint8_t *)(b + off[4]);
    v.child_action = (uint16_t *)(b + off[5]);
    v.child_visits = (uint32_t *)(b + off[6]);
    v.value = (double *)(b + off[7]);
    return v;
}

// A view as eight untyped pointers, in the order of records_sizes: array-by-array copies stay loops.
static inline void records_ptrs(const AzRecords &v, void *out[AZ_RECORD_ARRAYS]) {
    void *p[AZ_RECORD_ARRAYS] = {v.game_len, v.game_ret0, v.states, v.move, v.n_children, v.child_action, v.child_visits, v.value};
    for (int i = 0; i < AZ_RECORD_ARRAYS; i++) out[i] = p[i];
}
