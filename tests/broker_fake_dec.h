// broker_fake_dec.h - what tests/broker_harness.cpp tells the model decoder of tests/broker_fake_dec.cpp, and what it reads back.
#pragma once

#include <string>

#include "juicer_amd.h"

struct FakeCfg {
    int max_streams = 8, D = 4;
    int partial_interval = 0;           // > 0: a stream's list grows by one entry per this many frames (jd_stream_partial)
    int polls_per_command = 3;          // a posted command is through after this many jd_res_poll calls for its stream
    bool fail_start = false;            // jd_res_start fails
    int fail_stage_nth = 0;             // the n-th jd_res_stage_many fails (1-based; 0: none)
    int fail_post_nth = 0;              // the n-th jd_res_post fails, and the chunk it was to post is lost
    int err_stream = -1, err_frame = 0; // stream err_stream fails on the device when it reaches frame err_frame (>= 1) of an utterance
    int stop_every = 0;                 // a command stops short at every multiple of this many frames (stopped; jd_res_collect)
    int yield_after_polls = 0;          // jd_res_should_yield answers 1 once this many polls have been made since the kernel's start
    int end_after_polls = 0;            // the poll of this number (counted over the decoder's life) and those behind it, up to the
                                        // next jd_res_start, report the kernel as ended - once
};
struct FakeCounts {
    long long starts, stops, yields, collects, stage_calls, posts, polls, res_inits, res_finishes;   // jd_res_*
    long long inits, pushes, finishes, partials;                                                       // the streaming interface
};

jd_dec *fake_dec_create(const FakeCfg &cfg);
void fake_dec_destroy(jd_dec *d);
FakeCounts fake_dec_counts(jd_dec *d);
// the JD_BROKER_* knobs jd_dev_env finds (value null: unset)
void fake_env_set(const char *name, const char *value);
void fake_env_clear();
// the error a failed stream reports (jd_res_stream_error, jd_res_finish, jd_stream_finish)
enum { FAKE_STREAM_ERROR = JD_ENOMEM };
// the partial list the fake keeps for a stream of T frames under an interval: entry k is (label k + 1, time (k + 1) * interval - 1);
// a finished utterance has one more, (label 1000000 + T, time T - 1)
