// lg_policy_internal.h — what lg_estimator.hip needs from lg_policy.hip beyond the C ABI: the thread's error message (the one
// lg_mlp_last_error(NULL) returns) and the widths of the opaque network handles, to check that the stages of an estimator fit together.
#pragma once
#include <string>
#include "../../include/lgpolicy.h"

void lg_policy_set_error(const std::string& msg);
void lg_mlp_widths(const lg_mlp* m, int* layers, int* in, int* out, int* device);
void lg_rnn_widths(const lg_rnn* m, int* type, int* input, int* hidden, int* device);
