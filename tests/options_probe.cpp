// options_probe — llama_box_amd/csrc/options.h driven from a plain C++ program (tests/test_options_host.py compiles and runs it; no HIP, no GPU).
//   rows                 one line per option: key type default env-name-or-dash
//   env                  options_from_env over the defaults, then one line per option: key value
//   set K=V [K=V ...]    options_set one after the other on default options; after each a line: rc=<0|1> eq=<equal to the defaults> then every key=value
//   stats                one line per counter of a fresh backend: key value
//   helpers              env_flag / env_int / env_present against the four getenv idioms they replace, over unset, "", 0, 1, 2, x (exit 1 on a difference)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "options.h"

using namespace mi355x;

static void dump(const options & o, const char * sep, const char * end) {
#define MI_X(type, name, def, flag, env) printf("%s%s%d%s", #name, sep, (int) o.name, end);
    MI_OPTIONS(MI_X)
#undef MI_X
}

static int helpers() {
    static const char * const K = "MI355X_PROBE_KNOB";
    const char * const values[] = {nullptr, "", "0", "1", "2", "x"};
    int bad = 0;
    for (const char * v : values) {
        if (v) setenv(K, v, 1); else unsetenv(K);
        // the idioms as the launchers spelled them
        const bool on_unless_0 = !getenv("MI355X_PROBE_KNOB") || atoi(getenv("MI355X_PROBE_KNOB")) != 0;
        const bool off_unless_n = getenv("MI355X_PROBE_KNOB") && atoi(getenv("MI355X_PROBE_KNOB")) != 0;
        const int number = getenv("MI355X_PROBE_KNOB") ? atoi(getenv("MI355X_PROBE_KNOB")) : 7;
        const bool present = getenv("MI355X_PROBE_KNOB") != nullptr;
        const bool same = env_flag(K, true) == on_unless_0 && env_flag(K, false) == off_unless_n && env_int(K, 7) == number && env_present(K) == present;
        printf("%s flag_true=%d flag_false=%d int7=%d present=%d %s\n", v ? (v[0] ? v : "empty") : "unset", (int) env_flag(K, true), (int) env_flag(K, false), env_int(K, 7),
               (int) env_present(K), same ? "same" : "DIFFERENT");
        bad += !same;
    }
    return bad ? 1 : 0;
}

int main(int argc, char ** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    options o;
    if (cmd == "rows") {
#define MI_X(type, name, def, flag, env) printf("%s %s %d %s\n", #name, #type, (int) o.name, env ? option_env_name(#name).c_str() : "-");
        MI_OPTIONS(MI_X)
#undef MI_X
        return 0;
    }
    if (cmd == "env") {
        options_from_env(o);
        dump(o, " ", "\n");
        return 0;
    }
    if (cmd == "set") {
        for (int i = 2; i < argc; ++i) {
            const char * eq = strchr(argv[i], '=');
            if (!eq) return 2;
            const bool rc = options_set(o, std::string(argv[i], (size_t) (eq - argv[i])).c_str(), atoi(eq + 1));
            printf("rc=%d eq=%d ", (int) rc, (int) (o == options()));
            dump(o, "=", " ");
            printf("\n");
        }
        return 0;
    }
    if (cmd == "stats") {
        const stats st;
#define MI_X(name) { const int64_t * v = stats_find(st, #name); printf("%s %lld\n", #name, v == &st.name ? (long long) *v : -1LL); }
        MI_STATS(MI_X)
#undef MI_X
        return stats_find(st, "no_such_stat") ? 1 : 0;
    }
    if (cmd == "helpers") return helpers();
    fprintf(stderr, "usage: options_probe rows | env | set K=V ... | stats | helpers\n");
    return 2;
}
