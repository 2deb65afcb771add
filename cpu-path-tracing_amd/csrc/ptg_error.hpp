// ptg_error.hpp -- the thread-local message behind ptg_last_error
// (include/ptgpu.h) and the one way to set it: `return fail(code, msg);`.
// Shared by the host headers (scene_prep.hpp, launch_plan.hpp) and the C ABI
// in ptg_render.hip; a stand-alone program that includes them gets its own.
#pragma once

#include <string>

namespace ptg {

inline thread_local std::string g_last_error;

inline int fail(int code, const std::string &msg)
{
    g_last_error = msg;
    return code;
}

}  // namespace ptg
