// dev_switches.h - the one reader of the library's environment switches (INTEGRATION.md 4 describes each).  HIP-free.
// None is needed in production: they exist so that every data-dependent specialisation can be A/B-ed and tested.  Every
// switch is listed ONCE below with how it parses and the MOMENT at which it is read; tests set them between contexts of one
// process, so a call site asks for the switches of its own moment, when that moment comes, and keeps nothing.
// (PathTracer_HIP.cpp, the shim above the C ABI, is a library of its own and reads its own variables.)
#pragma once

#include <climits>
#include <cstdlib>
#include <cstring>

namespace ptmi_switches {

enum class Moment {
    kProcess,      // once per process, by the first ptmi_render call (only PTMI_SERIAL_LAUNCHES: an oddity, kept as it was)
    kSetup,        // ptmi_setup_context
    kUpload,       // ptmi_initialize_memory (ptmi_validate_scene too: the layout's part)
    kKernelKind,   // wherever the context asks "one path per lane?": at upload and by every render call
    kRenderCall,   // every ptmi_render / ptmi_render_snapshots call, per device
    kLaunch,       // every launch of the wavefront kernel
    kQueryLaunch,  // every launch of the ray-query kernel
    kGuideLaunch,  // every launch of the guide-buffer kernel
    kReadback,     // every gather of a snapshot (ptmi_read_image, ptmi_read_snapshot ...)
};

enum class Parse {
    kIsSet,       // 1 where the variable exists, whatever its value; else 0
    kFirstChar,   // the value's first character ('\0' for an empty value); kUnset without the variable
    kInteger,     // strtol, base 10, saturated to int; kUnset without the variable
    kReduceMode,  // kReduceRcclAlways for "rccl-always", kReduceRccl for any other "rccl..."; else ("peer", unset) 0
};
constexpr int kUnset = INT_MIN;
constexpr int kReduceRccl = 1, kReduceRcclAlways = 2;

struct Switches {
    int serial_launches = 0;
    int iterations_per_launch = kUnset, leaf_cull = kUnset;
    int generic_shading = 0, generic_triangles = 0, generic_boxes = 0, wide_records = 0, walk_nan_rays = 0;
    int literal_kernel = kUnset;
    int render_ahead = kUnset, render_ahead_calls = kUnset;
    int wide_workgroups = 0, random_give_up = kUnset;
    int query_max_blocks = kUnset, guide_max_blocks = kUnset;
    int reduce = 0;
};

struct SwitchRow {
    const char* name;
    Parse parse;
    Moment moment;
    int Switches::*field;
};
constexpr SwitchRow kSwitchTable[] = {
    {"PTMI_SERIAL_LAUNCHES", Parse::kIsSet, Moment::kProcess, &Switches::serial_launches},
    {"PTMI_ITERATIONS_PER_LAUNCH", Parse::kInteger, Moment::kSetup, &Switches::iterations_per_launch},
    {"PTMI_LEAF_CULL", Parse::kFirstChar, Moment::kSetup, &Switches::leaf_cull},
    {"PTMI_GENERIC_SHADING", Parse::kIsSet, Moment::kUpload, &Switches::generic_shading},
    {"PTMI_GENERIC_TRIANGLES", Parse::kIsSet, Moment::kUpload, &Switches::generic_triangles},
    {"PTMI_GENERIC_BOXES", Parse::kIsSet, Moment::kUpload, &Switches::generic_boxes},
    {"PTMI_WIDE_RECORDS", Parse::kIsSet, Moment::kUpload, &Switches::wide_records},
    {"PTMI_WALK_NAN_RAYS", Parse::kIsSet, Moment::kUpload, &Switches::walk_nan_rays},
    {"PTMI_LITERAL_KERNEL", Parse::kFirstChar, Moment::kKernelKind, &Switches::literal_kernel},
    {"PTMI_RENDER_AHEAD", Parse::kInteger, Moment::kRenderCall, &Switches::render_ahead},
    {"PTMI_RENDER_AHEAD_CALLS", Parse::kInteger, Moment::kRenderCall, &Switches::render_ahead_calls},
    {"PTMI_WIDE_WORKGROUPS", Parse::kIsSet, Moment::kLaunch, &Switches::wide_workgroups},
    {"PTMI_RANDOM_GIVE_UP", Parse::kFirstChar, Moment::kLaunch, &Switches::random_give_up},
    {"PTMI_QUERY_MAX_BLOCKS", Parse::kInteger, Moment::kQueryLaunch, &Switches::query_max_blocks},
    {"PTMI_GUIDE_MAX_BLOCKS", Parse::kInteger, Moment::kGuideLaunch, &Switches::guide_max_blocks},
    {"PTMI_REDUCE", Parse::kReduceMode, Moment::kReadback, &Switches::reduce},
};

// the value of one row, now
inline int read_row(const SwitchRow& row)
{
    const char* v = std::getenv(row.name);
    switch (row.parse) {
    case Parse::kIsSet: return v != nullptr;
    case Parse::kFirstChar: return v ? (int)(unsigned char)v[0] : kUnset;
    case Parse::kInteger: {
        if (!v) return kUnset;
        const long n = std::strtol(v, nullptr, 10);
        return n > INT_MAX ? INT_MAX : n <= INT_MIN ? INT_MIN + 1 : (int)n;
    }
    case Parse::kReduceMode:
        if (!v) return 0;
        if (std::strcmp(v, "rccl-always") == 0) return kReduceRcclAlways;
        return std::strncmp(v, "rccl", 4) == 0 ? kReduceRccl : 0;
    }
    return kUnset;
}

// The switches of `moment`, read now; every other field keeps its "unset" value.
inline Switches read_switches(Moment moment)
{
    Switches s;
    for (const SwitchRow& row : kSwitchTable)
        if (row.moment == moment) s.*row.field = read_row(row);
    return s;
}

// One switch by name (for a caller that is handed the name: stack_kernel_grid); kUnset for a name the table does not hold.
inline int read_switch(const char* name)
{
    for (const SwitchRow& row : kSwitchTable)
        if (std::strcmp(row.name, name) == 0) return read_row(row);
    return kUnset;
}

// a switch that holds a number: `fallback` where it is unset, clamped to [lo, hi]
inline int clamped(int value, int fallback, int lo, int hi)
{
    const int v = value == kUnset ? fallback : value;
    return v < lo ? lo : (v > hi ? hi : v);
}

}  // namespace ptmi_switches
