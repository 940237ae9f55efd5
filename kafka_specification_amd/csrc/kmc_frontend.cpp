// kmc_frontend.cpp — the "front end" section of include/kmc.h: what a TLC model configuration, a spec file, a canonical-byte
// state and a stock-TLC switch mean.  Both tlc-shaped command lines (kafka_specification_amd/tlc.py through ctypes,
// kmc_cli.cpp) ask here; nothing of it exists a second time.  Plain C++17 host code: no HIP, no handle, no environment.
//
// The reference repository ships no .cfg files (its .gitignore excludes *.toolbox), so the models/*.cfg twins are authored
// in this repository; names bind to KafkaReplication.tla:32-36 (constants) and :101,320,334,345 (invariants).
#include <dlfcn.h>

#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cerrno>
#include <cstring>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/kmc.h"

namespace kmc_engine {
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));   // sets kmc_last_error (kmc_engine_codeobj.cpp)
}
using kmc_engine::fail;

namespace {

__attribute__((format(printf, 1, 2))) std::string fmt(const char* f, ...) {
    char buf[8192];   // (a message holds at most one file name)
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// caller-owned text buffer: at most cap - 1 characters and a 0
void copy_out(const std::string& s, char* out, uint64_t cap) {
    if (!out || !cap) return;
    const size_t n = s.size() < cap - 1 ? s.size() : (size_t)(cap - 1);
    memcpy(out, s.data(), n);
    out[n] = 0;
}

bool is_word(const std::string& s) {
    for (char ch : s)
        if (!isalnum((unsigned char)ch) && ch != '_') return false;
    return !s.empty();
}

std::string trim(const std::string& s) {
    size_t a = 0, b = s.size();
    while (a < b && isspace((unsigned char)s[a])) ++a;
    while (b > a && isspace((unsigned char)s[b - 1])) --b;
    return s.substr(a, b - a);
}

// `\*` to the end of the line and `(* ... *)`; false: a `(*` that is never closed
bool strip_comments(const std::string& in, std::string* out) {
    for (size_t i = 0; i < in.size();) {
        if (in.compare(i, 2, "(*") == 0) {
            const size_t e = in.find("*)", i + 2);
            if (e == std::string::npos) return false;
            i = e + 2;
            *out += ' ';
        } else if (in.compare(i, 2, "\\*") == 0) {
            while (i < in.size() && in[i] != '\n') ++i;
        } else {
            *out += in[i++];
        }
    }
    return true;
}

// ---- the .cfg reader [TLC-recall] ----------------------------------------------------------------------------------
const char* const CFG_KEYWORDS[] = {"CONSTANT", "CONSTANTS", "INIT", "NEXT", "SPECIFICATION", "INVARIANT", "INVARIANTS",
                                    "CHECK_DEADLOCK", "CONSTRAINT", "CONSTRAINTS"};
// each one changes the set of distinct states, or asks for liveness
const char* const CFG_UNSUPPORTED[] = {"SYMMETRY", "ACTION_CONSTRAINT", "VIEW", "PROPERTY", "PROPERTIES", "ALIAS", "POSTCONDITION"};

template <size_t N>
bool among(const std::string& w, const char* const (&list)[N]) {
    for (const char* k : list)
        if (w == k) return true;
    return false;
}

struct CfgError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// a constant's value: an integer, TRUE / FALSE, a "string", a model value, or a set {v, ...} of those
struct Value {
    std::string text;                 // as written (strings without their quotes)
    bool is_int = false, is_set = false;
    long long number = 0;
    std::vector<std::string> elements;   // is_set: every element's text
};

Value parse_value(std::string tok) {
    Value v;
    tok = trim(tok);
    if (tok.size() >= 2 && tok.front() == '{' && tok.back() == '}') {
        v.is_set = true;
        v.text = tok;
        const std::string inner = trim(tok.substr(1, tok.size() - 2));
        for (size_t at = 0; !inner.empty() && at <= inner.size();) {
            const size_t comma = inner.find(',', at);
            v.elements.push_back(parse_value(inner.substr(at, comma == std::string::npos ? comma : comma - at)).text);
            at = comma == std::string::npos ? inner.size() + 1 : comma + 1;
        }
        return v;
    }
    if (tok.size() >= 2 && tok.front() == '"' && tok.back() == '"') {
        v.text = tok.substr(1, tok.size() - 2);
        return v;
    }
    v.text = tok;
    const size_t digits = tok[0] == '-' ? 1 : 0;
    if (tok.size() > digits && tok.find_first_not_of("0123456789", digits) == std::string::npos) {
        v.is_int = true;
        v.number = strtoll(tok.c_str(), nullptr, 10);   // (saturates: whoever needs the constant refuses it as out of range)
        v.text = std::to_string(v.number);              // 07 and 7 are one value
    }
    return v;
}

struct Cfg {
    std::map<std::string, Value> constants;
    std::vector<std::string> invariants, constraints;
    std::string init, next, specification;   // empty: not given
    int check_deadlock = 1;                   // TLC's default
};

std::vector<std::string> tokenize(const std::string& s) {
    std::vector<std::string> t;
    for (size_t i = 0; i < s.size();) {
        if (isspace((unsigned char)s[i])) { ++i; continue; }
        size_t e = std::string::npos;
        if (s[i] == '{') e = s.find('}', i);                       // a set, spaces and line ends included
        else if (s[i] == '"') e = s.find('"', i + 1);              // a string
        if (e != std::string::npos) e += 1;
        else if (s.compare(i, 2, "<-") == 0) e = i + 2;
        else if (s[i] == '=') e = i + 1;
        else for (e = i; e < s.size() && !isspace((unsigned char)s[e]) && s[e] != '='; ++e) {}
        t.push_back(s.substr(i, e - i));
        i = e;
    }
    return t;
}

Cfg parse_cfg(const std::string& text) {
    Cfg c;
    std::string bare;
    if (!strip_comments(text, &bare)) throw CfgError{"a (* comment is never closed"};
    const std::vector<std::string> t = tokenize(bare);
    std::string section;
    for (size_t i = 0; i < t.size(); ++i) {
        const std::string& w = t[i];
        if (among(w, CFG_UNSUPPORTED))
            throw CfgError{w + " is not supported (it changes the distinct-state count or asks for liveness)"};
        if (among(w, CFG_KEYWORDS)) {
            section = w;
        } else if (section == "CONSTANT" || section == "CONSTANTS") {
            if (i + 1 < t.size() && t[i + 1] == "<-")
                throw CfgError{"`" + w + " <- ...` (substitution by an operator of the spec) is not supported: no TLA+ is parsed, "
                               "so a replaced definition cannot be honoured; assign a value with `=`"};
            if (i + 1 >= t.size() || t[i + 1] != "=") throw CfgError{"expected `" + w + " = value` in CONSTANTS"};
            if (i + 2 >= t.size()) throw CfgError{"constant " + w + " has no value"};
            c.constants[w] = parse_value(t[i + 2]);
            i += 2;
        } else if (section == "INIT") {
            c.init = w;
        } else if (section == "NEXT") {
            c.next = w;
        } else if (section == "SPECIFICATION") {
            c.specification = w;
        } else if (section == "INVARIANT" || section == "INVARIANTS") {
            c.invariants.push_back(w);
        } else if (section == "CONSTRAINT" || section == "CONSTRAINTS") {
            c.constraints.push_back(w);
        } else if (section == "CHECK_DEADLOCK") {
            if (w != "TRUE" && w != "FALSE") throw CfgError{"CHECK_DEADLOCK takes TRUE or FALSE"};
            c.check_deadlock = w == "TRUE";
        } else {
            throw CfgError{"unexpected token " + w};
        }
    }
    return c;
}

const Value& need(const Cfg& c, const char* name) {
    const auto it = c.constants.find(name);
    if (it == c.constants.end()) throw CfgError{fmt("constant %s is not assigned in the .cfg", name)};
    return it->second;
}

long long need_int(const Cfg& c, const char* name, long long limit = INT32_MAX) {
    const Value& v = need(c, name);
    if (!v.is_int) throw CfgError{fmt("constant %s must be an integer, got %s", name, v.text.c_str())};
    if (v.number < -limit || v.number > limit) throw CfgError{fmt("constant %s is out of range", name)};
    return v.number;
}

const Value& need_distinct_set(const Cfg& c, const char* name) {
    const Value& v = need(c, name);
    if (!v.is_set || std::set<std::string>(v.elements.begin(), v.elements.end()).size() != v.elements.size())
        throw CfgError{fmt("%s must be a set of distinct model values", name)};
    return v;
}

bool holds(const Value& set, const std::string& element) {
    for (const std::string& e : set.elements)
        if (e == element) return true;
    return false;
}

void bind(const std::string& module, const Cfg& cfg, kmc_config* out) {
    if (module == "AsyncIsr")
        throw CfgError{"AsyncIsr.tla is unbounded (version: Nat, offsets: [Replicas -> Nat]); check it through the root module "
                       "models/MCAsyncIsr.tla, which adds CONSTRAINT StateConstraint"};
    // models/MCAsyncIsr.tla = AsyncIsr + the state constraint: the one root module whose lowered model carries another name
    int32_t model = module == "MCAsyncIsr" ? KMC_ASYNC_ISR : -1;
    std::string known;
    for (int32_t m = 0; m < KMC_ASYNC_ISR; ++m) {
        if (module == kmc_model_name(m)) model = m;
        known += std::string(kmc_model_name(m)) + ", ";
    }
    if (model < 0) throw CfgError{"module " + module + " has no lowered model; known: " + known + "MCAsyncIsr"};
    if (!cfg.constraints.empty() && model != KMC_ASYNC_ISR)
        throw CfgError{"CONSTRAINT is not supported for this module (it changes the distinct-state count)"};
    kmc_config c = *out;
    c.model = model;
    int n_invariants = 4;   // of kmc_model_invariant_name(model, .) this module knows
    if (model == KMC_IDSEQUENCE) {
        c.max_id = need_int(cfg, "MaxId", INT64_MAX - 1);
        n_invariants = 1;
    } else if (model == KMC_ASYNC_ISR) {   // AsyncIsr.tla:22-29 + MaxVersion / StateConstraint of models/MCAsyncIsr.tla
        const Value& reps = need_distinct_set(cfg, "Replicas");
        if (!holds(reps, need(cfg, "Leader").text))
            throw CfgError{"Leader must be an element of Replicas (ASSUME Leader \\in Replicas, AsyncIsr.tla:29)"};
        if (need_int(cfg, "MaxOffset") <= 0) throw CfgError{"MaxOffset must be positive (ASSUME MaxOffset > 0, AsyncIsr.tla:28)"};
        if (cfg.constraints != std::vector<std::string>{"StateConstraint"})
            throw CfgError{"MCAsyncIsr needs exactly `CONSTRAINT StateConstraint`: AsyncIsr is unbounded without it"};
        c.n_replicas = (int32_t)reps.elements.size();   // (the engine's replica 0 is Leader: the spec tells the others apart by nothing)
        c.log_size = need_int(cfg, "MaxOffset");
        c.max_leader_epoch = need_int(cfg, "MaxVersion");
        n_invariants = 3;
    } else if (model == KMC_FINITE_REPLICATED_LOG) {
        const Value &reps = need(cfg, "Replicas"), &recs = need(cfg, "LogRecords");
        if (!reps.is_set || !recs.is_set) throw CfgError{"Replicas and LogRecords must be sets of model values"};
        need(cfg, "Nil");
        c.n_replicas = (int32_t)reps.elements.size();
        c.n_log_records = (int32_t)recs.elements.size();
        c.log_size = need_int(cfg, "LogSize");
        n_invariants = 1;
    } else {
        const Value& reps = need_distinct_set(cfg, "Replicas");
        if (holds(reps, "NONE"))
            throw CfgError{"Replicas must not contain \"NONE\" (ASSUME None \\notin Replicas, KafkaReplication.tla:42)"};
        c.n_replicas = (int32_t)reps.elements.size();
        c.log_size = need_int(cfg, "LogSize");
        c.max_records = need_int(cfg, "MaxRecords");
        c.max_leader_epoch = need_int(cfg, "MaxLeaderEpoch");
    }
    if (!cfg.specification.empty() && cfg.specification != "Spec") throw CfgError{"only SPECIFICATION Spec is known"};
    if (!cfg.specification.empty() && !(cfg.init.empty() && cfg.next.empty()))
        // [TLC-recall] TLC refuses the combination too (EC.TLC_CONFIG_NOT_BOTH_SPEC_AND_INIT)
        throw CfgError{"a .cfg gives either SPECIFICATION or INIT / NEXT, not both"};
    if ((!cfg.init.empty() && cfg.init != "Init") || (!cfg.next.empty() && cfg.next != "Next"))
        throw CfgError{"only INIT Init / NEXT Next are known"};
    c.invariant_mask = 0;
    for (const std::string& inv : cfg.invariants) {
        int bit = -1;
        for (int k = 0; k < n_invariants; ++k)
            if (inv == kmc_model_invariant_name(model, k)) bit = k;
        if (bit < 0) throw CfgError{"unknown invariant " + inv + " for module " + module};
        c.invariant_mask |= 1u << bit;
    }
    c.check_deadlock = cfg.check_deadlock;
    *out = c;
}

// ---- spec identity: sha256 of the ten modules of the reference revision (sha256sum *.tla) ----------------------------------
const char* const SPEC_SHA256[][2] = {
    {"AsyncIsr", "6c29fa0de4174c9a36b1b933b43df115f53254f727cdf6b05b1c6306e77f3e46"},
    {"FiniteReplicatedLog", "cc6193fcc9bc75be6ce2b4ab9719d9bb645c0e0441e53fda630097e13edde747"},
    {"IdSequence", "bf8a9f74c8ccad8aa2ee4139df4297942f9a8a429afffb2e1f032833b6912654"},
    {"KafkaReplication", "80fffc6c9e430106cb0be059f542239fa85079ffe5834493f96cbadfe122ed9a"},
    {"KafkaTruncateToHighWatermark", "97b38e8c1d41113173784cee59c884b54554a9608ac7ddad442f80eed7af6d35"},
    {"Kip101", "77a8ea39557ae7e19c975eb62cc1b4253761a22426c562c1e891fc361f918f6f"},
    {"Kip279", "9568ffd395b77367722757b8a3aab999b682ab657e4fb13d41629c3696b4e39f"},
    {"Kip320", "4f2dccca13414af26dbebeffbdb105b46973f55c79a46c04be76cde73aa963ca"},
    {"Kip320FirstTry", "b2985bc5dad379d15cc88e838f0e3bce8e232a52a197c7f5dcd941821467d705"},
    {"Util", "56a9514e28ac684657a91456f1f8985351bf23c9ec29d65e69a65987cfc9b385"},
};
const char* const STANDARD_MODULES[] = {"Integers", "Naturals", "Sequences", "FiniteSets", "TLC", "Reals", "Bags"};

std::string sha256_hex(const std::string& data) {  // FIPS 180-4
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
        0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
        0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
        0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
        0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
        0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    std::string m = data;
    const uint64_t bits = (uint64_t)data.size() * 8;
    m += (char)0x80;
    while (m.size() % 64 != 56) m += (char)0;
    for (int i = 7; i >= 0; --i) m += (char)(bits >> (8 * i));
    auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
    for (size_t off = 0; off < m.size(); off += 64) {
        uint32_t w[64];
        for (int i = 0; i < 16; ++i)
            w[i] = ((uint32_t)(unsigned char)m[off + 4 * i] << 24) | ((uint32_t)(unsigned char)m[off + 4 * i + 1] << 16) |
                   ((uint32_t)(unsigned char)m[off + 4 * i + 2] << 8) | (uint32_t)(unsigned char)m[off + 4 * i + 3];
        for (int i = 16; i < 64; ++i) {
            const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
            const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; ++i) {
            const uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25), ch = (e & f) ^ (~e & g);
            const uint32_t t1 = hh + S1 + ch + K[i] + w[i];
            const uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22), maj = (a & b) ^ (a & c) ^ (b & c);
            const uint32_t t2 = S0 + maj;
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    char out[65];
    for (int i = 0; i < 8; ++i) snprintf(out + 8 * i, 9, "%08x", h[i]);
    return out;
}

bool slurp(const std::string& path, std::string* out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    char buf[4096];
    size_t n;
    out->clear();
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, n);
    fclose(f);
    return true;
}

std::string dir_of(const std::string& path) {
    const size_t slash = path.find_last_of('/');
    return slash == std::string::npos ? "." : path.substr(0, slash);
}

std::string module_of(const std::string& path) {   // a/b/Kip320.tla -> Kip320
    const size_t slash = path.find_last_of('/');
    std::string name = path.substr(slash == std::string::npos ? 0 : slash + 1);
    const size_t dot = name.find_last_of('.');
    if (dot != std::string::npos && dot > 0) name.resize(dot);
    return name;
}

// the sha256 a module of the lowered revision must have; empty: not one of them
std::string expected_sha256(const std::string& module) {
    for (const auto& e : SPEC_SHA256)
        if (module == e[0]) return e[1];
    Dl_info info;
    std::string mine;   // authored in this repository: the copy in models/, beside the package this library lies in
    if (module == "MCAsyncIsr" && dladdr((void*)&kmc_spec_check, &info) && info.dli_fname &&
        slurp(dir_of(info.dli_fname) + "/../models/MCAsyncIsr.tla", &mine))
        return sha256_hex(mine);
    return "";
}

// the module names a module EXTENDS or INSTANCEs
std::vector<std::string> imports_of(const std::string& text) {
    std::string t;
    std::vector<std::string> names;
    if (!strip_comments(text, &t)) return names;
    auto keyword_at = [&](size_t at, size_t len) {   // a whole word
        return (at == 0 || !(isalnum((unsigned char)t[at - 1]) || t[at - 1] == '_')) &&
               (at + len >= t.size() || !(isalnum((unsigned char)t[at + len]) || t[at + len] == '_'));
    };
    for (size_t at = t.find("EXTENDS"); at != std::string::npos; at = t.find("EXTENDS", at + 7)) {
        if (!keyword_at(at, 7)) continue;
        const size_t e = t.find('\n', at);
        const std::string line = t.substr(at + 7, (e == std::string::npos ? t.size() : e) - at - 7) + ",";
        for (size_t a = 0, comma; (comma = line.find(',', a)) != std::string::npos; a = comma + 1) {
            const std::string name = trim(line.substr(a, comma - a));
            if (is_word(name)) names.push_back(name);
        }
    }
    for (size_t at = t.find("INSTANCE"); at != std::string::npos; at = t.find("INSTANCE", at + 8)) {
        if (!keyword_at(at, 8)) continue;
        size_t i = at + 8;
        while (i < t.size() && isspace((unsigned char)t[i])) ++i;
        std::string name;
        while (i < t.size() && (isalnum((unsigned char)t[i]) || t[i] == '_')) name += t[i++];
        if (i > at + 8 && !name.empty()) names.push_back(name);
    }
    return names;
}

// ---- canonical bytes -> TLA+ text, the way TLC prints a trace state (layout: include/kmc.h) --------------------------
std::string name_set(unsigned mask, int n, char prefix) {
    std::string s = "{";
    for (int r = 0; r < n; ++r)
        if (mask >> r & 1u) s += (s.size() > 1 ? ", " : "") + (prefix + std::to_string(r + 1));
    return s + "}";
}

std::string format_async_isr(int N, int V, const uint8_t* b) {   // AsyncIsr.tla:31-35; replica 1 is `Leader`
    const int rb = ((1 << N) + 7) / 8;
    const uint8_t* q = b + 6 + N;
    const uint8_t* u = q + (V + 1) * rb;
    std::string offsets, requests, updates;
    for (int r = 0; r < N; ++r) offsets += fmt("%sr%d :> %d", r ? " @@ " : "", r + 1, b[6 + r]);
    for (int v = 0; v <= V; ++v)
        for (int m = 0; m < (1 << N); ++m)
            if (q[v * rb + (m >> 3)] >> (m & 7) & 1)
                requests += fmt("%s[isr |-> %s, version |-> %d]", requests.empty() ? "" : ", ", name_set(m, N, 'r').c_str(), v);
    for (int v = 1; v <= b[1] && v <= V + 1; ++v)
        updates += fmt("%s[isr |-> %s, version |-> %d]", v > 1 ? ", " : "", name_set(u[v - 1], N, 'r').c_str(), v);
    return fmt("/\\ controllerState = [isr |-> %s, version |-> %d]\n", name_set(b[0], N, 'r').c_str(), b[1]) +
           fmt("/\\ leaderState = [isr |-> %s, version |-> %d, pendingIsr |-> %s, pendingVersion |-> %d, offsets |-> (",
               name_set(b[2], N, 'r').c_str(), b[3], name_set(b[4], N, 'r').c_str(), b[5] - 1) +
           offsets + ")]\n/\\ requests = {" + requests + "}\n/\\ updates = {" + updates + "}";
}

std::string format_replicated_log(int N, int L, const uint8_t* b) {
    std::string s = "logs = (";
    for (int r = 0; r < N; ++r) {
        const uint8_t* k = b + r * (1 + L);
        s += fmt("%sr%d :> [endOffset |-> %d, records |-> <<", r ? " @@ " : "", r + 1, k[0]);
        for (int o = 0; o < L; ++o) s += (o ? ", " : "") + (k[1 + o] ? "x" + std::to_string(k[1 + o]) : std::string("Nil"));
        s += ">>]";
    }
    return s + ")";
}

std::string format_kafka(int N, int L, int E, const uint8_t* b) {
    const int rs = 5 + L;
    auto leader = [](int x) { return x == 0 ? std::string("\"NONE\"") : "b" + std::to_string(x); };
    std::string logs, states, requests;
    for (int r = 0; r < N; ++r) {
        const uint8_t* k = b + r * rs;
        logs += fmt("%sb%d :> [endOffset |-> %d, records |-> <<", r ? " @@ " : "", r + 1, k[0]);
        for (int o = 0; o < L; ++o) {
            const int code = k[5 + o];
            logs += (o ? ", " : "") + (code == 0 ? std::string("-1") : fmt("[id |-> %d, epoch |-> %d]", (code - 1) / (E + 1), (code - 1) % (E + 1)));
        }
        logs += ">>]";
        states += fmt("%sb%d :> [hw |-> %d, leaderEpoch |-> %d, leader |-> %s, isr |-> %s]", r ? " @@ " : "", r + 1, k[1], k[2] - 1,
                      leader(k[3]).c_str(), name_set(k[4], N, 'b').c_str());
    }
    const uint8_t* g = b + N * rs;
    for (int e = 0; e < g[1] && e <= E; ++e)
        requests += fmt("%s[leaderEpoch |-> %d, leader |-> %s, isr |-> %s]", e ? ", " : "", e, leader(g[5 + 2 * e]).c_str(),
                        name_set(g[6 + 2 * e], N, 'b').c_str());
    return "/\\ replicaLog = (" + logs + ")\n/\\ replicaState = (" + states + ")\n" +
           fmt("/\\ nextRecordId = %d\n/\\ nextLeaderEpoch = %d\n", g[0], g[1]) + "/\\ leaderAndIsrRequests = {" + requests + "}\n" +
           fmt("/\\ quorumState = [leaderEpoch |-> %d, leader |-> %s, isr |-> %s]", g[2] - 1, leader(g[3]).c_str(),
               name_set(g[4], N, 'b').c_str());
}

// ---- stock TLC's other switches [TLC-recall] ----------------------------------------------------------------------------
struct Switch {
    const char* flag;
    int32_t switch_class;
    const char* why;
};
const Switch TLC_SWITCHES[] = {
    // what does not change the question is accepted and ignored with a note (a wrapper script written for `java tlc2.TLC`
    // keeps working) ...
    {"-modelcheck", KMC_SWITCH_IGNORED, "model checking is the only mode"},
    {"-cleanup", KMC_SWITCH_IGNORED, "no states directory is written"},
    {"-nowarning", KMC_SWITCH_IGNORED, "no TLA+ is evaluated, so no evaluation warnings exist"},
    {"-terse", KMC_SWITCH_IGNORED, "values are printed in full"},
    {"-tool", KMC_SWITCH_IGNORED, "no tool-mode message codes"},
    {"-gzip", KMC_SWITCH_IGNORED, "checkpoints are not compressed"},
    {"-debug", KMC_SWITCH_IGNORED, "no debug output"},
    {"-noGenerateSpecTE", KMC_SWITCH_IGNORED, "no trace-expression spec is generated"},
    {"-difftrace", KMC_SWITCH_IGNORED, "traces print every variable of every state"},
    {"-metadir", KMC_SWITCH_IGNORED_VALUE, "nothing is written there"},
    {"-userFile", KMC_SWITCH_IGNORED_VALUE, "the lowered models print nothing"},
    {"-fpmem", KMC_SWITCH_IGNORED_VALUE, "the fingerprint table lives in HBM: -table SLOTS sizes it"},
    {"-fpbits", KMC_SWITCH_IGNORED_VALUE, "one table, no partitioning by bits"},
    {"-maxSetSize", KMC_SWITCH_IGNORED_VALUE, "no set is enumerated at run time"},
    {"-coverage", KMC_SWITCH_IGNORED_VALUE, "action coverage is not collected"},
    {"-lncheck", KMC_SWITCH_IGNORED_VALUE, "no liveness checking"},
    // ... what asks for another mode of operation is refused: silently dropping it would answer a different question
    {"-simulate", KMC_SWITCH_REFUSED, "random simulation is another mode of TLC; only exhaustive breadth-first model checking is implemented"},
    {"-depth", KMC_SWITCH_REFUSED, "it belongs to -simulate"},
    {"-seed", KMC_SWITCH_REFUSED, "it belongs to -simulate"},
    {"-aril", KMC_SWITCH_REFUSED, "it belongs to -simulate"},
    {"-dump", KMC_SWITCH_REFUSED, "the reachable states stay on the GPU (kmc_frontier_states gives a level's states through the C ABI)"},
    {"-view", KMC_SWITCH_REFUSED, "a VIEW changes the distinct-state count"},
    {"-dfid", KMC_SWITCH_REFUSED, "depth-first iterative deepening is another search order"},
    {"-generateSpecTE", KMC_SWITCH_REFUSED, "no trace-expression spec is generated"},
};

}  // namespace

extern "C" {

int kmc_cfg_bind(const char* module, const char* cfg_text, kmc_config* out) {
    if (!module || !cfg_text || !out) return fail(KMC_E_ARG, "kmc_cfg_bind: null argument");
    try {
        bind(module, parse_cfg(cfg_text), out);
    } catch (const std::exception& e) {
        return fail(KMC_E_ARG, "%s", e.what());
    }
    return KMC_OK;
}

int kmc_spec_check(const char* spec_path, char* msgs, uint64_t cap) {
    const std::string path = spec_path ? spec_path : "";
    std::string text, report;
    int status = 0;
    if (!slurp(path, &text)) {
        report = path + " does not exist: checking the built-in lowering of " + module_of(path) +
                 " (reference revision, sha256 table in libkmc.so)\n";
        status = 1;
    }
    std::vector<std::string> todo = {module_of(path)};
    std::set<std::string> seen;
    while (status != 1 && !todo.empty()) {
        const std::string mod = todo.back();
        todo.pop_back();
        if (among(mod, STANDARD_MODULES) || !seen.insert(mod).second) continue;
        const std::string file = dir_of(path) + "/" + mod + ".tla";
        if (!slurp(file, &text)) {
            report += "module " + mod + ": " + file + " not found (not verified)\n";
            continue;
        }
        const std::string want = expected_sha256(mod), got = sha256_hex(text);
        if (want.empty()) {
            report += "module " + mod + ": not a module of the lowered revision\n";
            status = 2;
        } else if (want != got) {
            report += fmt("module %s: %s differs from the revision the kernels were lowered from (sha256 %.16s..., expected %.16s...)\n",
                          mod.c_str(), file.c_str(), got.c_str(), want.c_str());
            status = 2;
        }
        for (const std::string& name : imports_of(text)) todo.push_back(name);
    }
    if (!report.empty()) report.pop_back();
    copy_out(report, msgs, cap);
    return status;
}

int64_t kmc_format_state(const kmc_config* cfg, const uint8_t* canon, uint64_t canon_len, char* out, uint64_t cap) {
    if (!cfg || !canon) return fail(KMC_E_ARG, "kmc_format_state: null argument"), -1;
    const int N = cfg->n_replicas, L = cfg->log_size, E = cfg->max_leader_epoch;
    const bool plain = cfg->model == KMC_IDSEQUENCE;
    if (cfg->model < 0 || cfg->model > KMC_ASYNC_ISR || (!plain && (N < 1 || N > 8 || L < 0 || L > 255 || E < 0 || E > 255)))
        return fail(KMC_E_ARG, "kmc_format_state: constants out of range (model %d, %d replicas, log size %d, epochs %d)", cfg->model, N, L, E), -1;
    const uint64_t need = plain                                     ? 8
                          : cfg->model == KMC_ASYNC_ISR             ? 6 + N + (uint64_t)(E + 1) * (((1 << N) + 7) / 8) + E + 1
                          : cfg->model == KMC_FINITE_REPLICATED_LOG ? (uint64_t)N * (1 + L)
                                                                    : (uint64_t)N * (5 + L) + 5 + 2 * (E + 1);
    if (canon_len < need)
        return fail(KMC_E_ARG, "kmc_format_state: %llu canonical bytes given, these constants have %llu", (unsigned long long)canon_len,
                    (unsigned long long)need), -1;
    std::string s;
    if (plain) {
        uint64_t v;
        memcpy(&v, canon, 8);
        s = "nextId = " + std::to_string(v);
    } else {
        s = cfg->model == KMC_ASYNC_ISR ? format_async_isr(N, E, canon)
            : cfg->model == KMC_FINITE_REPLICATED_LOG ? format_replicated_log(N, L, canon) : format_kafka(N, L, E, canon);
    }
    copy_out(s, out, cap);
    return (int64_t)s.size();
}

const char* kmc_tlc_switch(const char* flag, int32_t* switch_class) {
    const Switch* hit = nullptr;
    for (const Switch& s : TLC_SWITCHES)
        if (flag && !strcmp(flag, s.flag)) hit = &s;
    if (switch_class) *switch_class = hit ? hit->switch_class : KMC_SWITCH_NONE;
    return hit ? hit->why : nullptr;
}

int kmc_collision_report(uint64_t distinct, uint64_t generated, uint64_t orbit_representatives, int32_t wide, int32_t finished_ok,
                         char* out, uint64_t cap) {
    // the seen-set holds the representatives: they are what can collide, and what was probed for
    uint64_t stored = distinct, probed = generated;
    if (orbit_representatives && distinct) {
        stored = orbit_representatives;
        probed = (uint64_t)((unsigned __int128)generated * stored / distinct);
    }
    // (products of two counts as exact integers, rounded once)
    auto scaled = [](uint64_t a, uint64_t b, int bits) { return std::ldexp((double)((unsigned __int128)a * b), -bits); };
    std::string s;
    int rc = 0;
    if (wide) {
        // every entry also holds a second, independent 64-bit hash of the state: two states are only merged when both words agree
        s = "The seen-set stores 128 bits per state (the fingerprint and an independent check word); probability that two "
            "distinct states were merged:\n" +
            fmt("  birthday bound on the stored entries:  val = %.2E", scaled(stored, stored, 129));
    } else {
        // [TLC-recall: "calculated (optimistic)" = distinct x (generated - distinct) / 2^64], plus the birthday bound n^2 / 2^65
        const double birthday = scaled(stored, stored, 65);
        s = "The seen-set stores 64-bit fingerprints; estimates of the probability that not all reachable states were "
            "checked because two distinct states had the same fingerprint:\n" +
            fmt("  calculated (optimistic):  val = %.2E\n", scaled(stored, probed > stored ? probed - stored : 0, 64)) +
            fmt("  birthday bound on the stored fingerprints:  val = %.2E", birthday);
        if (birthday > KMC_FP128_ADVICE_ABOVE) {
            // (Kip320 3/6/6/3: 6,452,700,520 states, birthday bound 1.1 — the 64-bit search returns one state fewer)
            s += fmt("\n  Recommendation: that bound is above %g: counts of this size are only bit-exact with 128-bit entries - re-run "
                     "with -fp128 (or, on the Kafka modules, -symmetry: a sixth of the stored fingerprints at three brokers).",
                     KMC_FP128_ADVICE_ABOVE);
            // A FINISHED search whose count is more likely wrong than not must not look like a success to a script: BASELINE's
            // target is the bit-identical count (a verdict that already failed keeps its own code).
            if (finished_ok) {
                rc = KMC_EXIT_UNCERTIFIED;
                s += fmt("\nWarning: the distinct-state count of this run is NOT certified (64-bit fingerprints, birthday bound %.2E > "
                         "%g): exit code %d.", birthday, KMC_FP128_ADVICE_ABOVE, KMC_EXIT_UNCERTIFIED);
            }
        }
    }
    copy_out(s, out, cap);
    return rc;
}

// The switches of random simulation, for both command lines: -walks N [-walk-depth D] [-walk-seed S], each given as the text
// that followed it (NULL: the switch was not given).  Stock TLC's -simulate / -depth / -seed stay refused (TLC_SWITCHES).
static bool whole_number(const char* t, uint64_t* v) {
    if (!t || !*t) return false;
    for (const char* q = t; *q; ++q)
        if (*q < '0' || *q > '9') return false;
    errno = 0;
    *v = strtoull(t, nullptr, 10);
    return errno == 0;
}
int kmc_walk_switches(const char* walks, const char* depth, const char* seed, kmc_sim_config* out, int32_t* asked) {
    if (!out || !asked) return fail(KMC_E_ARG, "kmc_walk_switches: null argument");
    *asked = walks != nullptr;
    if (!walks) {
        if (depth) return fail(KMC_E_ARG, "-walk-depth belongs to -walks N: say how many random walks to run");
        if (seed) return fail(KMC_E_ARG, "-walk-seed belongs to -walks N: say how many random walks to run");
        return KMC_OK;
    }
    uint64_t n = 0, d = 100, sd = 0;
    if (!whole_number(walks, &n)) return fail(KMC_E_ARG, "-walks needs a whole number of walks, not '%s'", walks);
    if (n == 0) return fail(KMC_E_ARG, "-walks 0: a batch holds at least 1 walk");
    if (depth && (!whole_number(depth, &d) || d == 0 || d > (1u << 20)))
        return fail(KMC_E_ARG, "-walk-depth needs a number of states between 1 and %u, not '%s'", 1u << 20, depth);
    if (seed && !whole_number(seed, &sd)) return fail(KMC_E_ARG, "-walk-seed needs a whole number below 2^64, not '%s'", seed);
    memset(out, 0, sizeof *out);
    out->n_walks = n;
    out->depth = (uint32_t)d;
    out->seed = sd;
    return KMC_OK;
}

// What both command lines print around a batch of walks: closing = 0 the opening line, 1 the lines after it (the verdict and
// the behaviour are the caller's, as for a search; so are the names of the model's actions: this unit stands alone).  Lines joined by '\n'; returns the length of the whole text.
int64_t kmc_sim_report(const kmc_config* cfg, const kmc_sim_config* sim, const kmc_sim_result* res, int32_t closing,
                       const char* const* action_names, int32_t n_actions, char* out, uint64_t cap) {
    if (!cfg || !sim || (closing && !res)) return fail(KMC_E_ARG, "kmc_sim_report: null argument"), -1;
    std::string s;
    if (!closing) {
        s = fmt("Running Random Simulation with seed %llu: %llu walks of at most %u states on GPU %d.", (unsigned long long)sim->seed,
                (unsigned long long)sim->n_walks, sim->depth ? sim->depth : 100u, cfg->device);
    } else {
        s = fmt("Progress: %llu walks run in %llu launches, %llu states checked.\n", (unsigned long long)res->walks,
                (unsigned long long)res->launches, (unsigned long long)res->states_generated);
        s += fmt("The number of states generated: %llu\n", (unsigned long long)res->states_generated);
        s += fmt("Simulation using seed %llu, walks %llu to %llu.\n", (unsigned long long)sim->seed, (unsigned long long)sim->first_walk,
                 (unsigned long long)(sim->first_walk + res->walks - 1));
        s += "Steps taken per action:";
        for (int k = 0; action_names && k < n_actions && k < KMC_MAX_KINDS; ++k)
            s += fmt(" %s %llu", action_names[k], (unsigned long long)res->action_taken[k]);
        s += fmt("\n%llu walks ended on a state without successors; the longest walk has %llu states.",
                 (unsigned long long)res->ended_early, (unsigned long long)res->longest_walk);
    }
    copy_out(s, out, cap);
    return (int64_t)s.size();
}

int32_t kmc_uncertified_policy(double* advice_above) {
    if (advice_above) *advice_above = KMC_FP128_ADVICE_ABOVE;
    return KMC_EXIT_UNCERTIFIED;
}

}  // extern "C"
