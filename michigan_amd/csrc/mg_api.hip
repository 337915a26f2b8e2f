// mg_api.hip -- ABI bookkeeping for libmichigan_hip.so
#include "mg_common.h"
#include "mg_options.h"

thread_local char g_mg_err[512] = {0};
mg_option_values g_mg_options = mg_option_defaults();

extern "C" int mg_abi_version(void) { return MG_ABI_VERSION; }
extern "C" const char* mg_last_error(void) { return g_mg_err; }
extern "C" int mg_sizeof_desc(int32_t which)
{
    return which == 0 ? (int)sizeof(mg_conv_desc) : which == 1 ? (int)sizeof(mg_wgrad_desc) : which == 2 ? (int)sizeof(mg_grad_slot) : which == 3 ? (int)sizeof(mg_pack_job) : which == 4 ? (int)sizeof(mg_sn_layer) : which == 5 ? (int)sizeof(mg_norm_apply2_desc) : which == 6 ? (int)sizeof(mg_pyramid_desc) : which == 7 ? (int)sizeof(mg_feat_moment_desc) : -1;
}

// the row of a switch that exists in this build, or nullptr
static const mg_option_row* option_row(int32_t key)
{
    for (const mg_option_row& r : MG_OPTIONS)
        if (r.key == key && (MG_PROBES || !r.probes)) return &r;
    return nullptr;
}

#if MG_PROBES
int conv_halo_set_probe(unsigned long long addr);        // mg_conv_halo.hip
int wgrad3x3_set_probe(unsigned long long addr);         // mg_wgrad3x3.hip
#endif

extern "C" int mg_set_option(int32_t key, int32_t value)
{
    const mg_option_row* r = option_row(key);
    if (r == nullptr || value < r->min || value > r->max || value % r->step != 0)
        return mg_fail(MG_ERR_ARG, "mg_set_option: unknown key/value %d/%d", key, value);
    g_mg_options.v[key] = value;
#if MG_PROBES
    if (key == MG_OPT_PROBE_ADDR_HI) {                   // both halves are in: hand the stamp buffer to the stamped kernels
        const unsigned long long a = ((unsigned long long)(unsigned)value << 32) | (unsigned)mg_opt(MG_OPT_PROBE_ADDR_LO);
        const int rc = conv_halo_set_probe(a);
        return rc != MG_OK ? rc : wgrad3x3_set_probe(a);
    }
#endif
    return MG_OK;
}

extern "C" int mg_get_option(int32_t key, int32_t* value)
{
    const mg_option_row* r = option_row(key);
    if (r == nullptr || value == nullptr) return mg_fail(MG_ERR_ARG, "mg_get_option: unknown key %d or null pointer", key);
    *value = g_mg_options.v[key];
    return MG_OK;
}
