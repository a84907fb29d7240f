// The error boundary of every extern "C" entry point of libccz: the handle's device is current for the call (and the
// caller's restored after it), ccz::Error becomes its code with the message kept in the handle, a failed host
// allocation CCZ_ENOMEM, anything else CCZ_EHIP.
#pragma once

#include <new>

#include "ops.h"

#define CCZ_GUARD(h, ...)                   \
  if (!(h)) return CCZ_EINVAL;              \
  try {                                     \
    ::ccz::DeviceScope ccz_scope_(h);       \
    __VA_ARGS__;                            \
    return CCZ_OK;                          \
  } catch (const ccz::Error& e) {           \
    (h)->err = e.msg;                       \
    return e.code;                          \
  } catch (const std::bad_alloc&) {         \
    (h)->err = "host allocation failed";    \
    return CCZ_ENOMEM;                      \
  } catch (...) {                           \
    (h)->err = "unknown internal error";    \
    return CCZ_EHIP;                        \
  }
