// mg_options.h -- the one list of the library's tuning switches (enum mg_option in michigan_hip.h says what each means).
// mg_set_option / mg_get_option (mg_api.hip) are lookups in MG_OPTIONS; the launchers read a switch with mg_opt(key).
// A new switch is its enumerator in michigan_hip.h plus one row here.  Host side only: kernels get what they need
// through their argument structs.
#pragma once
#include <stdint.h>
#include "michigan_hip.h"
#ifndef MG_PROBES
#define MG_PROBES 0        // 1: measurement builds (stamped / truncated kernel variants + their switches); tools/build_variant.py
#endif

struct mg_option_row { int key, def, min, max, step; bool probes; };    // value in [min, max] and a multiple of step; probes: MG_PROBES builds only

constexpr mg_option_row MG_OPTIONS[] = {
    //  key                          default  min        max        step  probes
    {MG_OPT_CONV_BIGTILES,           1,       0,         1,         1,    false},
    {MG_OPT_CONV_HALO,               1,       0,         1,         1,    false},
    {MG_OPT_WGRAD3X3,                1,       0,         1,         1,    false},
    {MG_OPT_CONV_HALO_BIG,           1,       0,         1,         1,    false},
    {MG_OPT_CONV_SPLITK,             1,       0,         1,         1,    false},
    {MG_OPT_CONV_THIN,               2,       0,         2,         1,    false},
    {MG_OPT_CONV_WIDE,               1,       0,         1,         1,    false},
    {MG_OPT_CONV_DOT,                2,       0,         2,         1,    false},
    {MG_OPT_PROBE_HALO_VARIANT,      0,       0,         6,         1,    true},
    {MG_OPT_PROBE_WGRAD3X3,          0,       0,         1,         1,    true},
    {MG_OPT_PROBE_ADDR_LO,           0,       INT32_MIN, INT32_MAX, 1,    true},
    {MG_OPT_PROBE_ADDR_HI,           0,       INT32_MIN, INT32_MAX, 1,    true},
    {MG_OPT_PROBE_NOXPRE,            0,       0,         1,         1,    true},
    {MG_OPT_WGRAD_MIN_STAGES,        32,      1,         1024,      1,    false},
    {MG_OPT_NORM_BWD_VEC,            1,       0,         1,         1,    false},
    {MG_OPT_PROBE_HALO_LDSPAD,       0,       0,         80 * 1024, 1,    true},
    {MG_OPT_CONV_HALO64,             1,       0,         1,         1,    false},
    {MG_OPT_PROBE_HALO64_DBG,        0,       0,         7,         1,    true},
    {MG_OPT_WGRAD3X3_STRIPE,         64,      0,         4096,      32,   false},
};

struct mg_option_values { int v[MG_OPT_END]; };
constexpr mg_option_values mg_option_defaults()
{
    mg_option_values s = {};
    for (const mg_option_row& r : MG_OPTIONS) s.v[r.key] = r.def;
    return s;
}

extern mg_option_values g_mg_options;                                     // mg_api.hip
static inline int mg_opt(int key) { return g_mg_options.v[key]; }
