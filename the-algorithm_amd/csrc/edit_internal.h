// edit_internal.h -- what the two translation units of include/edit_ann.h share: the thread-local error channel (owned by
// the host-only edit_host.cpp, so that edit_last_error() reads one message whichever unit failed) and the host-side checks of
// caller data that come before any device call.
#pragma once
#include <stdint.h>

#include <string>

#include "../../include/edit_ann.h"
#include "abi_guard.h"

namespace edit_host {

int fail(int code, const std::string &message);

// offsets [n + 1] into n_chars elements: present, 0 <= offsets[0], non-decreasing, offsets[n] <= n_chars, every length at
// most EDIT_MAX_LENGTH.  `what` names the strings in the message.  n = 0 passes with anything.
int check_csr(const char *what, int64_t n, const int64_t *offsets, const float *chars, int64_t n_chars);

// The plain two-row dynamic programme over IEEE ==.
int32_t plain_distance(const float *a, int la, const float *b, int lb);

}  // namespace edit_host

#define EDIT_ABI_CATCH catch (...) { return abi_guard::caught(edit_host::fail, EDIT_ENOMEM, EDIT_EINTERNAL); }
