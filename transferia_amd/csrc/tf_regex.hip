// tf_regex.hip — regex_replace_transformer (pkg/transformer/registry/regex_replace/transformer.go).
//
// Host: the pattern compiler (Go regexp / regexp/syntax restated for the subset include/tfgpu.h lists; everything else is
// refused by name) and the replaceRule compiler (Regexp.expand / extract).  Device: Regexp.ReplaceAll per text cell — a
// Pike VM (priority-ordered thread lists with capture slots, leftmost-first) run by one lane per cell, a length pass, the
// shared scan, a write pass.  No backtracking, no recursion: one search costs at most (cell length + 1) steps of at most
// `program size` threads each, and the searches of a cell together at most (length + 1) * (program size + 16) + 1024 steps — a cell that needs
// more (a pattern that is quadratic in Go too), a cell above TFGPU_REGEX_MAX_CELL and a result of 4 GiB are refused after the length pass.
#include <algorithm>

#include "tf_plan.hpp"
#include "tf_devcol.hpp"
#include "tf_rows.hpp"

namespace tf {

// ============================================================================
// host: pattern → program
// ============================================================================
namespace {
constexpr uint32_t RUNE_MAX = 0x10FFFF, RUNE_ERROR = 0xFFFD;
constexpr int NO_MAX = -1;

[[noreturn]] void rx_bad(const std::string &m) { throw Error(TFGPU_ERR_CONFIG, "unable to compile match regexp: " + m); }
[[noreturn]] void rx_unsupported(const std::string &what) {
  throw Error(TFGPU_ERR_UNSUPPORTED, "regex_replace_transformer: " + what + " is outside the device subset of RE2 syntax: keep the transformer on the host");
}

enum NodeKind { N_EMPTY, N_CHAR, N_CLASS, N_ANYNOTNL, N_CAT, N_ALT, N_REP, N_GROUP, N_NOCAP, N_ASSERT };
struct Node {
  int kind = N_EMPTY;
  uint32_t c = 0;                                     // N_CHAR: the rune; N_ASSERT: RxAssert
  std::vector<std::pair<uint32_t, uint32_t>> ranges;  // N_CLASS: sorted, merged, negation applied
  std::vector<int> kids;
  int min = 0, max = 0;  // N_REP
  bool lazy = false;
  bool counted = false;  // N_REP written {n}, {n,} or {n,m}
  int idx = 0;           // N_GROUP: capture index (1-based)
};

using Ranges = std::vector<std::pair<uint32_t, uint32_t>>;
void ranges_norm(Ranges &r) {
  std::sort(r.begin(), r.end());
  Ranges o;
  for (auto &x : r) {
    if (!o.empty() && x.first <= o.back().second + 1) o.back().second = std::max(o.back().second, x.second);
    else o.push_back(x);
  }
  r.swap(o);
}
void ranges_negate(Ranges &r) {
  ranges_norm(r);
  Ranges o;
  uint32_t next = 0;
  for (auto &x : r) { if (x.first > next) o.push_back({next, x.first - 1}); next = x.second + 1; }
  if (next <= RUNE_MAX) o.push_back({next, RUNE_MAX});
  r.swap(o);
}
void perl_class(char k, Ranges &into) {  // \d \w \s and their negations as Go defines them (ASCII)
  Ranges r;
  switch (k | 0x20) {
    case 'd': r = {{'0', '9'}}; break;
    case 'w': r = {{'0', '9'}, {'A', 'Z'}, {'_', '_'}, {'a', 'z'}}; break;
    case 's': r = {{'\t', '\n'}, {'\f', '\r'}, {' ', ' '}}; break;
  }
  if (!(k & 0x20)) ranges_negate(r);
  into.insert(into.end(), r.begin(), r.end());
}

struct Parser {
  std::vector<uint32_t> t;  // the pattern's runes
  size_t i = 0;
  std::vector<Node> nodes;
  int ngroups = 0;

  explicit Parser(const std::string &src) {
    const uint8_t *s = (const uint8_t *)src.data();
    const size_t n = src.size();
    for (size_t k = 0; k < n;) {  // strict UTF-8 (syntax.checkUTF8)
      uint32_t b = s[k], cp; int need;
      if (b < 0x80) { t.push_back(b); k++; continue; }
      if (b >= 0xC2 && b <= 0xDF) { need = 1; cp = b & 0x1F; }
      else if (b >= 0xE0 && b <= 0xEF) { need = 2; cp = b & 0x0F; }
      else if (b >= 0xF0 && b <= 0xF4) { need = 3; cp = b & 0x07; }
      else rx_bad("invalid UTF-8");
      if (k + (size_t)need >= n) rx_bad("invalid UTF-8");
      for (int j = 1; j <= need; j++) { uint32_t c = s[k + (size_t)j]; if ((c & 0xC0) != 0x80) rx_bad("invalid UTF-8"); cp = cp << 6 | (c & 0x3F); }
      if ((need == 2 && (cp < 0x800 || (cp >= 0xD800 && cp <= 0xDFFF))) || (need == 3 && (cp < 0x10000 || cp > RUNE_MAX))) rx_bad("invalid UTF-8");
      if (cp == RUNE_ERROR) rx_unsupported("a literal U+FFFD in the pattern");
      t.push_back(cp);
      k += (size_t)need + 1;
    }
  }
  bool more() const { return i < t.size(); }
  uint32_t peek(size_t k = 0) const { return i + k < t.size() ? t[i + k] : 0xFFFFFFFFu; }
  int add(Node n) { nodes.push_back(std::move(n)); return (int)nodes.size() - 1; }
  static std::string show(uint32_t c) { std::string o; if (c < 0x80) o += (char)c; else o = "U+" + std::to_string(c); return o; }

  // {n} {n,} {n,m} at t[i] == '{' (syntax.parseRepeat); false: the brace is a literal
  bool parse_repeat(size_t &adv, int &mn, int &mx) const {
    size_t k = i + 1;
    auto num = [&](int &out) {
      size_t b = k;
      long v = 0;
      while (k < t.size() && t[k] >= '0' && t[k] <= '9') { if (v < 100000000) v = v * 10 + (long)(t[k] - '0'); k++; }
      if (k == b) return false;
      if (k - b >= 2 && t[b] == '0') return false;  // leading zeros are no number
      out = v >= 100000000 ? 100000000 : (int)v;
      return true;
    };
    if (!num(mn)) return false;
    mx = mn;
    if (k < t.size() && t[k] == ',') {
      k++;
      if (k < t.size() && t[k] == '}') mx = NO_MAX;
      else if (!num(mx)) return false;
    }
    if (k >= t.size() || t[k] != '}') return false;
    adv = k + 1 - i;
    return true;
  }

  int parse_alt(int depth) {
    if (depth > 64) rx_unsupported("groups nested deeper than 64 levels");
    std::vector<int> alts;
    alts.push_back(parse_cat(depth));
    while (more() && peek() == '|') { i++; alts.push_back(parse_cat(depth)); }
    if (alts.size() == 1) return alts[0];
    Node n; n.kind = N_ALT; n.kids = alts;
    return add(std::move(n));
  }
  int parse_cat(int depth) {
    std::vector<int> items;
    while (more() && peek() != '|' && peek() != ')') {
      int a = parse_atom(depth);
      bool repeated = false;
      for (;;) {
        int mn = 0, mx = 0; size_t adv = 1;
        bool counted = false;
        const uint32_t c = peek();
        if (c == '*') { mn = 0; mx = NO_MAX; }
        else if (c == '+') { mn = 1; mx = NO_MAX; }
        else if (c == '?') { mn = 0; mx = 1; }
        else if (c == '{' && parse_repeat(adv, mn, mx)) {
          if (mn > 1000 || mx > 1000) rx_unsupported("a repeat count above 1000");
          if (mx != NO_MAX && mn > mx) rx_bad("invalid repeat count");
          counted = true;
        } else break;
        if (repeated) rx_bad("invalid nested repetition operator");  // (syntax.Perl: a** is an error, not a doubled star)
        i += adv;
        Node r; r.kind = N_REP; r.min = mn; r.max = mx; r.counted = counted; r.kids = {a};
        if (peek() == '?') { r.lazy = true; i++; }
        a = add(std::move(r));
        repeated = true;
      }
      items.push_back(a);
    }
    if (items.empty()) return add(Node{});
    if (items.size() == 1) return items[0];
    Node n; n.kind = N_CAT; n.kids = items;
    return add(std::move(n));
  }
  int make_char(uint32_t c) { Node n; n.kind = N_CHAR; n.c = c; return add(std::move(n)); }
  int make_class(Ranges r, bool negate) {
    if (negate) ranges_negate(r); else ranges_norm(r);
    Node n; n.kind = N_CLASS; n.ranges = std::move(r);
    return add(std::move(n));
  }
  int make_assert(uint32_t k) { Node n; n.kind = N_ASSERT; n.c = k; return add(std::move(n)); }

  // a backslash escape that stands for ONE rune, in or outside a class; i is at the character after the backslash
  uint32_t escape_rune() {
    const uint32_t c = t[i++];
    switch (c) {
      case 't': return '\t'; case 'n': return '\n'; case 'r': return '\r'; case 'f': return '\f'; case 'v': return '\v';
      case 'x': {
        if (peek() == '{') rx_unsupported("the escape \\x{...}");
        uint32_t v = 0;
        for (int k = 0; k < 2; k++) {
          const uint32_t h = peek();
          int d = (h >= '0' && h <= '9') ? (int)(h - '0') : (h >= 'a' && h <= 'f') ? (int)(h - 'a' + 10) : (h >= 'A' && h <= 'F') ? (int)(h - 'A' + 10) : -1;
          if (d < 0) rx_bad("invalid escape sequence: \\x");
          v = v * 16 + (uint32_t)d; i++;
        }
        return v;
      }
    }
    if (c < 0x80 && !((c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'))) return c;  // punctuation stands for itself
    if (c >= '1' && c <= '7' && peek() >= '0' && peek() <= '7') rx_unsupported("an octal escape");
    if (c >= '1' && c <= '9') rx_bad("invalid escape sequence: \\" + show(c));                                  // a backreference
    if (c == 'p' || c == 'P') rx_unsupported("the Unicode class \\p{...}");
    if (c == 'C') rx_unsupported("\\C");
    if (c == 'Q' || c == 'E') rx_unsupported("\\Q...\\E");
    if (c == '0') rx_unsupported("an octal escape");
    rx_unsupported("the escape \\" + show(c));
  }

  int parse_class() {  // i is behind '['
    Ranges r;
    bool negate = false;
    if (peek() == '^') { negate = true; i++; }
    bool first = true;
    for (;;) {
      if (!more()) rx_bad("missing closing ]");
      uint32_t c = peek();
      if (c == ']' && !first) { i++; break; }
      first = false;
      if (c == '[' && peek(1) == ':') rx_unsupported("a POSIX class [[:...:]]");
      uint32_t lo;
      if (c == '\\') {
        i++;
        if (!more()) rx_bad("trailing backslash at end of expression");
        const uint32_t e = peek();
        if (e == 'd' || e == 'D' || e == 'w' || e == 'W' || e == 's' || e == 'S') { i++; perl_class((char)e, r); continue; }
        lo = escape_rune();
      } else { lo = c; i++; }
      uint32_t hi = lo;
      if (peek() == '-' && peek(1) != ']' && i + 1 < t.size()) {
        i++;
        uint32_t h = peek();
        if (h == '\\') {
          i++;
          if (!more()) rx_bad("trailing backslash at end of expression");
          const uint32_t e = peek();
          if (e == 'd' || e == 'D' || e == 'w' || e == 'W' || e == 's' || e == 'S') rx_bad("invalid character class range");
          hi = escape_rune();
        } else { hi = h; i++; }
        if (hi < lo) rx_bad("invalid character class range");
      }
      r.push_back({lo, hi});
    }
    return make_class(std::move(r), negate);
  }

  int parse_atom(int depth) {
    const uint32_t c = t[i];
    switch (c) {
      case '*': case '+': case '?': rx_bad("missing argument to repetition operator: " + show(c));
      case '{': {
        size_t adv; int mn, mx;
        if (parse_repeat(adv, mn, mx)) rx_bad("missing argument to repetition operator");
        i++; return make_char('{');
      }
      case '(': {
        i++;
        bool capture = true;
        if (peek() == '?') {
          const uint32_t k = peek(1);
          if (k == ':') { capture = false; i += 2; }
          else if (k == '=' || k == '!') rx_bad("invalid or unsupported Perl syntax: (?" + show(k));
          else if (k == '<' && (peek(2) == '=' || peek(2) == '!')) rx_bad("invalid or unsupported Perl syntax: (?<" + show(peek(2)));
          else if (k == 'P' || k == '<') rx_unsupported("a named group");
          else {
            std::string f = "(?";
            for (size_t q = 1; q < 8 && peek(q) != 0xFFFFFFFFu && peek(q) != ')' && peek(q) != ':'; q++) f += show(peek(q));
            rx_unsupported("the flag group " + f + ")");
          }
        }
        int idx = 0;
        if (capture) idx = ++ngroups;
        const int body = parse_alt(depth + 1);
        if (!more() || peek() != ')') rx_bad("missing closing )");
        i++;
        Node n; n.kind = capture ? N_GROUP : N_NOCAP; n.idx = idx; n.kids = {body};
        return add(std::move(n));
      }
      case '[': i++; return parse_class();
      case '.': { i++; Node n; n.kind = N_ANYNOTNL; return add(std::move(n)); }
      case '^': i++; return make_assert(RXA_BEGIN_TEXT);
      case '$': i++; return make_assert(RXA_END_TEXT);  // no flags: the end of the text only
      case '\\': {
        i++;
        if (!more()) rx_bad("trailing backslash at end of expression");
        const uint32_t e = peek();
        switch (e) {
          case 'A': i++; return make_assert(RXA_BEGIN_TEXT);
          case 'z': i++; return make_assert(RXA_END_TEXT);
          case 'b': i++; return make_assert(RXA_WORD_BOUNDARY);
          case 'B': i++; return make_assert(RXA_NO_WORD_BOUNDARY);
          case 'd': case 'D': case 'w': case 'W': case 's': case 'S': { i++; Ranges r; perl_class((char)e, r); return make_class(std::move(r), false); }
        }
        return make_char(escape_rune());
      }
    }
    i++;
    return make_char(c);
  }

  // syntax.repeatIsValid: the counts of nested {n,m} repeats multiply, and the product may not pass 1000
  bool repeats_valid(int ni, int n) const {
    const Node &nd = nodes[(size_t)ni];
    if (nd.kind == N_REP && nd.counted) {
      int m = nd.max;
      if (m == 0) return true;
      if (m < 0) m = nd.min;
      if (m > n) return false;
      if (m > 0) n /= m;
    }
    for (int k : nd.kids) if (!repeats_valid(k, n)) return false;
    return true;
  }
  bool can_be_empty(int ni) const {
    const Node &n = nodes[(size_t)ni];
    switch (n.kind) {
      case N_EMPTY: case N_ASSERT: return true;
      case N_CHAR: case N_CLASS: case N_ANYNOTNL: return false;
      case N_CAT: for (int k : n.kids) if (!can_be_empty(k)) return false; return true;
      case N_ALT: for (int k : n.kids) if (can_be_empty(k)) return true; return false;
      case N_GROUP: case N_NOCAP: return can_be_empty(n.kids[0]);
      case N_REP: return n.min == 0 || can_be_empty(n.kids[0]);
    }
    return true;
  }
};

struct Emitter {
  const Parser &ps;
  RegexProg &out;
  int max_ref;
  uint32_t pc() const { return (uint32_t)out.inst.size(); }
  uint32_t put(uint32_t op, uint32_t x = 0, uint32_t y = 0, uint32_t c = 0) {
    if (out.inst.size() >= (size_t)TFGPU_REGEX_MAX_PROG)
      rx_unsupported("a pattern that compiles to more than " + std::to_string(TFGPU_REGEX_MAX_PROG) + " instructions");
    out.inst.push_back(RxInst{op, x, y, c});
    return pc() - 1;
  }
  void emit(int ni) {
    const Node &n = ps.nodes[(size_t)ni];
    switch (n.kind) {
      case N_EMPTY: return;
      case N_CHAR: put(RX_CHAR, pc() + 1, 0, n.c); return;
      case N_ANYNOTNL: put(RX_ANYNOTNL, pc() + 1); return;
      case N_CLASS: {
        if (n.ranges.size() == 1 && n.ranges[0].first == n.ranges[0].second) { put(RX_CHAR, pc() + 1, 0, n.ranges[0].first); return; }
        if (n.ranges.size() == 1 && n.ranges[0].first == 0 && n.ranges[0].second == RUNE_MAX) { put(RX_ANY, pc() + 1); return; }
        const uint32_t first = (uint32_t)out.ranges.size() / 2;
        for (auto &r : n.ranges) { out.ranges.push_back(r.first); out.ranges.push_back(r.second); }
        if (out.ranges.size() / 2 > (size_t)TFGPU_REGEX_MAX_RANGES)
          rx_unsupported("character classes with more than " + std::to_string(TFGPU_REGEX_MAX_RANGES) + " ranges in all");
        put(RX_CLASS, pc() + 1, first, (uint32_t)n.ranges.size());  // (an empty class, [^\x00-\x{10FFFF}], matches nothing: zero pairs)
        return;
      }
      case N_ASSERT: put(RX_ASSERT, pc() + 1, 0, n.c); return;
      case N_CAT: for (int k : n.kids) emit(k); return;
      case N_NOCAP: emit(n.kids[0]); return;
      case N_GROUP:
        if (n.idx > max_ref) { emit(n.kids[0]); return; }  // the rule never reads it
        put(RX_SAVE, pc() + 1, 0, (uint32_t)(2 * n.idx));
        emit(n.kids[0]);
        put(RX_SAVE, pc() + 1, 0, (uint32_t)(2 * n.idx + 1));
        return;
      case N_ALT: {
        std::vector<uint32_t> jmps;
        for (size_t k = 0; k < n.kids.size(); k++) {
          if (k + 1 < n.kids.size()) {
            const uint32_t s = put(RX_SPLIT, pc() + 1);
            emit(n.kids[k]);
            jmps.push_back(put(RX_JMP));
            out.inst[s].y = pc();
          } else emit(n.kids[k]);
        }
        for (uint32_t j : jmps) out.inst[j].x = pc();
        return;
      }
      case N_REP: {
        const int body = n.kids[0];
        if (n.max == NO_MAX) {
          if (ps.can_be_empty(body)) rx_unsupported(std::string("a ") + (n.min == 0 ? "*" : n.min == 1 ? "+" : "{n,}") + " whose body can match the empty string");
          if (n.min == 0) {  // L: split(body, end); body; jmp L
            const uint32_t s = put(RX_SPLIT);
            emit(body);
            put(RX_JMP, s);
            out.inst[s].x = n.lazy ? pc() : s + 1;
            out.inst[s].y = n.lazy ? s + 1 : pc();
          } else {           // x{n,} = n-1 copies, then L: body; split(L, next)
            for (int k = 1; k < n.min; k++) { const uint32_t at = pc(); emit(body); if (pc() == at) break; }  // (a body without instructions: once is all of them)
            const uint32_t l = pc();
            emit(body);
            const uint32_t s = put(RX_SPLIT);
            out.inst[s].x = n.lazy ? s + 1 : l;
            out.inst[s].y = n.lazy ? l : s + 1;
          }
          return;
        }
        for (int k = 0; k < n.min; k++) { const uint32_t at = pc(); emit(body); if (pc() == at) break; }
        std::vector<uint32_t> splits;  // x{n,m} = n copies, then (x(x(x)?)?)?: every skip leaves the whole tail
        for (int k = n.min; k < n.max; k++) { splits.push_back(put(RX_SPLIT)); emit(body); }
        for (uint32_t s : splits) {
          out.inst[s].x = n.lazy ? pc() : s + 1;
          out.inst[s].y = n.lazy ? s + 1 : pc();
        }
        return;
      }
    }
  }
};

// Regexp.expand / extract (regexp.go) over the rule, once
void compile_rule(const std::string &rule, int ngroups, RegexProg &out) {
  if (rule.size() > (size_t)TFGPU_REGEX_MAX_RULE) rx_unsupported("a replaceRule longer than " + std::to_string(TFGPU_REGEX_MAX_RULE) + " bytes");
  auto lit = [&](const char *p, size_t n) {
    if (!n) return;
    if (!out.segs.empty() && out.segs.back().group < 0 && out.segs.back().off + out.segs.back().len == out.lits.size()) out.segs.back().len += (uint32_t)n;
    else out.segs.push_back(RxSeg{-1, (uint32_t)out.lits.size(), (uint32_t)n});
    out.lits.append(p, n);
  };
  const char *s = rule.data();
  const size_t n = rule.size();
  size_t i = 0;
  auto name_char = [](unsigned char c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_'; };
  while (i < n) {
    size_t d = i;
    while (d < n && s[d] != '$') d++;
    lit(s + i, d - i);
    if (d >= n) break;
    i = d + 1;  // behind the '$'
    if (i < n && s[i] == '$') { lit("$", 1); i++; continue; }
    size_t k = i;
    const bool brace = k < n && s[k] == '{';
    if (brace) k++;
    const size_t b = k;
    while (k < n && name_char((unsigned char)s[k])) k++;
    // Go's name runs over unicode.IsLetter / IsDigit: a non-ASCII letter here would join the name there
    if (k < n && (unsigned char)s[k] >= 0x80) rx_unsupported("a non-ASCII character directly behind a $name in replaceRule");
    if (k == b || (brace && (k >= n || s[k] != '}'))) { lit("$", 1); continue; }  // malformed: the $ is raw text
    const std::string name(s + b, k - b);
    i = brace ? k + 1 : k;
    long num = 0;
    for (char c : name) { if (c < '0' || c > '9' || num >= 100000000) { num = -1; break; } num = num * 10 + (c - '0'); }
    if (name[0] == '0' && name.size() > 1) num = -1;
    if (num >= 0 && num <= ngroups) out.segs.push_back(RxSeg{(int32_t)num, 0, 0});
    // (anything else — a group the pattern does not have, a name: named groups are refused — expands to nothing)
  }
}
}  // namespace

RegexProg regex_compile(const std::string &pattern, const std::string &rule) {
  Parser ps(pattern);
  const int root = ps.parse_alt(0);
  if (ps.more()) rx_bad("unexpected )");
  if (!ps.repeats_valid(root, 1000)) rx_unsupported("nested repeats whose counts multiply to a repeat count above 1000");
  if (ps.ngroups > TFGPU_REGEX_MAX_GROUPS) rx_unsupported("more than " + std::to_string(TFGPU_REGEX_MAX_GROUPS) + " capture groups");
  RegexProg out;
  out.ngroups = ps.ngroups;
  compile_rule(rule, ps.ngroups, out);
  int max_ref = 0;
  for (auto &sg : out.segs) max_ref = std::max(max_ref, (int)sg.group);
  out.nslots = 2 * (1 + max_ref);
  Emitter em{ps, out, max_ref};
  out.start = 0;
  em.emit(root);
  em.put(RX_MATCH);
  return out;
}

// ============================================================================
// device: Regexp.ReplaceAll per cell
// ============================================================================
constexpr uint32_t RX_NONE = 0xFFFFFFFFu;  // a capture slot no SAVE has written; the rune read at the end of the text
constexpr int RX_MAX_SLOTS = 2 * (1 + TFGPU_REGEX_MAX_GROUPS);
constexpr int RX_BLOCK = 256;
constexpr size_t RX_LDS_BUDGET = 56 * 1024;  // dynamic LDS of one workgroup (beside the 4 KiB program copy)
static_assert(TFGPU_REGEX_MAX_PROG <= 128, "RxSeen is two 64-bit words");

struct RxParams {
  const uint32_t *in_off; const uint8_t *in_data; const uint8_t *validity; int64_t n;
  const RxInst *inst; const uint32_t *ranges; const RxSeg *segs; const uint8_t *lits;  // one uploaded table
  uint32_t ninst, npairs, start, nslots, nsegs, stack_cap;
  uint32_t *ws; uint32_t lanes;  // thread lists and the add stack of every resident lane, lane-interleaved (HBM form; the LDS form keeps a workgroup's in LDS)
  uint32_t *out_len;             // length pass
  const uint32_t *out_off; uint8_t *out_data;  // write pass
  uint32_t *flags;               // RXF_* bits, or-ed by the lanes
};

// utf8.DecodeRune: an invalid or truncated sequence is U+FFFD of width 1
__device__ __forceinline__ uint32_t rx_decode(const uint8_t *t, uint32_t pos, uint32_t len, uint32_t &w) {
  const uint32_t b0 = t[pos];
  w = 1;
  if (b0 < 0x80) return b0;
  if (b0 < 0xC2 || b0 > 0xF4) return 0xFFFD;
  const uint32_t need = b0 < 0xE0 ? 2u : b0 < 0xF0 ? 3u : 4u;
  if (len - pos < need) return 0xFFFD;
  const uint32_t b1 = t[pos + 1];
  const uint32_t lo = b0 == 0xE0 ? 0xA0u : b0 == 0xF0 ? 0x90u : 0x80u, hi = b0 == 0xED ? 0x9Fu : b0 == 0xF4 ? 0x8Fu : 0xBFu;
  if (b1 < lo || b1 > hi) return 0xFFFD;
  if (need == 2) { w = 2; return (b0 & 0x1F) << 6 | (b1 & 0x3F); }
  const uint32_t b2 = t[pos + 2];
  if ((b2 & 0xC0) != 0x80) return 0xFFFD;
  if (need == 3) { w = 3; return (b0 & 0x0F) << 12 | (b1 & 0x3F) << 6 | (b2 & 0x3F); }
  const uint32_t b3 = t[pos + 3];
  if ((b3 & 0xC0) != 0x80) return 0xFFFD;
  w = 4;
  return (b0 & 0x07) << 18 | (b1 & 0x3F) << 12 | (b2 & 0x3F) << 6 | (b3 & 0x3F);
}
__device__ __forceinline__ bool rx_word(uint32_t b) { return (b >= '0' && b <= '9') || (b >= 'a' && b <= 'z') || (b >= 'A' && b <= 'Z') || b == '_'; }

// A lane's working memory: two thread lists of `ninst` threads (pc + capture slots) and rx_add's stack, word w of lane l at [w * lanes + l] so
// that the lanes of a wave touch neighbouring words.  LDSWS: it fits the workgroup's LDS (short programs, few slots); else a workspace in HBM.
TF_DYNAMIC_LDS(uint32_t, rx_lds);
template <bool LDSWS>
struct RxLane {
  const RxInst *inst;      // LDS
  const uint32_t *ranges;  // LDS
  uint32_t *ws; size_t lanes, lane;
  uint32_t ninst, nslots, stride;  // stride = 1 + nslots words per thread: pc, slots
  uint32_t stack_base, stack_cap;
  __device__ __forceinline__ uint32_t &at(uint32_t word) const {
    if (LDSWS) return rx_lds[word * (uint32_t)lanes + (uint32_t)lane];
    return ws[(size_t)word * lanes + lane];
  }
  __device__ __forceinline__ uint32_t thread_word(uint32_t list, uint32_t e, uint32_t k) const { return (list * ninst + e) * stride + k; }
};

// A byte below 0x80 is always a rune of its own (DecodeRune never takes it into a sequence), so whether the rune before / at q is a
// word character is a question about one byte each
__device__ __forceinline__ bool rx_assert_ok(uint32_t kind, const uint8_t *t, uint32_t len, uint32_t q) {
  if (kind == RXA_BEGIN_TEXT) return q == 0;
  if (kind == RXA_END_TEXT) return q == len;
  const bool before = q > 0 && rx_word(t[q - 1]), after = q < len && rx_word(t[q]);
  return (before != after) == (kind == RXA_WORD_BOUNDARY);
}

// regexp.(*machine).add without the recursion: follows the empty-width instructions from pc0 in priority order and appends every
// rune-consuming (or MATCH) instruction it reaches to `list` with a copy of `cap`.  `seen` holds the pcs this list has met (each at most
// once), so the stack — one entry per pending SPLIT branch or SAVE to undo, and the first — never grows past #SPLIT + #SAVE + 1.
// what a lane reports in RxParams::flags
constexpr uint32_t RXF_MATCHED = 1, RXF_INTERNAL = 2, RXF_BUDGET = 4, RXF_CELL = 8, RXF_4GIB = 16;

struct RxSeen {  // the pcs a thread list has met: two words picked by compare, so that they stay in registers
  uint64_t w0 = 0, w1 = 0;
  __device__ __forceinline__ bool test(uint32_t pc) const { return ((pc < 64 ? w0 : w1) >> (pc & 63)) & 1; }
  __device__ __forceinline__ void set(uint32_t pc) { const uint64_t b = 1ull << (pc & 63); w0 |= pc < 64 ? b : 0; w1 |= pc < 64 ? 0 : b; }
};
template <bool LDSWS>
__device__ __forceinline__ void rx_add(const RxLane<LDSWS> &L, uint32_t list, uint32_t &count, RxSeen &seen, uint32_t pc0, const uint8_t *t, uint32_t len, uint32_t q,
                                       uint32_t *cap, uint32_t &fault) {
  uint32_t sp = 0;
  L.at(L.stack_base) = pc0; L.at(L.stack_base + 1) = RX_NONE; sp = 1;
  while (sp > 0) {
    sp--;
    uint32_t pc = L.at(L.stack_base + 2 * sp);
    const uint32_t old = L.at(L.stack_base + 2 * sp + 1);
    if (pc & 0x80000000u) { cap[pc & 0xFFu] = old; continue; }  // leave a SAVE: its slot reads as before
    for (;;) {
      if (seen.test(pc)) break;
      seen.set(pc);
      const RxInst in = L.inst[pc];
      if (in.op == RX_JMP) { pc = in.x; continue; }
      if (in.op == RX_SPLIT) {
        if (sp >= L.stack_cap) { fault |= RXF_INTERNAL; break; }
        L.at(L.stack_base + 2 * sp) = in.y; L.at(L.stack_base + 2 * sp + 1) = RX_NONE; sp++;
        pc = in.x; continue;
      }
      if (in.op == RX_SAVE) {
        if (sp >= L.stack_cap) { fault |= RXF_INTERNAL; break; }
        L.at(L.stack_base + 2 * sp) = 0x80000000u | in.c; L.at(L.stack_base + 2 * sp + 1) = cap[in.c]; sp++;
        cap[in.c] = q;
        pc = in.x; continue;
      }
      if (in.op == RX_ASSERT) {
        if (!rx_assert_ok(in.c, t, len, q)) break;
        pc = in.x; continue;
      }
      if (count >= L.ninst) { fault |= RXF_INTERNAL; break; }
      L.at(L.thread_word(list, count, 0)) = pc;
      for (uint32_t k = 0; k < L.nslots; k++) L.at(L.thread_word(list, count, 1 + k)) = cap[k];
      count++;
      break;
    }
  }
}

template <bool LDSWS>
__device__ __forceinline__ bool rx_consumes(const RxLane<LDSWS> &L, const RxInst &in, uint32_t c) {
  switch (in.op) {
    case RX_CHAR: return c == in.c;
    case RX_ANY: return true;
    case RX_ANYNOTNL: return c != '\n';
    case RX_CLASS:
      for (uint32_t k = 0; k < in.c; k++) {
        const uint32_t lo = L.ranges[2 * (in.y + k)], hi = L.ranges[2 * (in.y + k) + 1];
        if (c < lo) return false;  // (sorted)
        if (c <= hi) return true;
      }
      return false;
  }
  return false;
}

// One leftmost-first search from `from`, with the whole cell as context (regexp.(*machine).match).  m[0 .. nslots) receives the match.
template <bool LDSWS>
__device__ __forceinline__ bool rx_search(const RxLane<LDSWS> &L, uint32_t start_pc, const uint8_t *t, uint32_t len, uint32_t from, uint32_t *m, uint32_t &fault, uint64_t &budget) {
  uint32_t cap[RX_MAX_SLOTS];
  RxSeen seen_c, seen_n;
  uint32_t cur = 0, nc = 0;
  bool matched = false;
  for (uint32_t pos = from;;) {
    if (nc == 0 && matched) break;
    if (budget == 0) { fault |= RXF_BUDGET; return false; }  // the cell's searches together may take (len + 1) * (ninst + 16) + 1024 steps
    budget--;
    if (!matched) {
      for (uint32_t k = 0; k < L.nslots; k++) cap[k] = RX_NONE;
      cap[0] = pos;
      rx_add(L, cur, nc, seen_c, start_pc, t, len, pos, cap, fault);
    }
    uint32_t w = 0, c = RX_NONE;
    if (pos < len) c = rx_decode(t, pos, len, w);
    uint32_t nn = 0;
    seen_n = RxSeen();
    for (uint32_t e = 0; e < nc; e++) {
      const uint32_t pc = L.at(L.thread_word(cur, e, 0));
      const RxInst in = L.inst[pc];
      if (in.op == RX_MATCH) {  // first-match mode: the threads behind this one have lower priority and are cut off
        for (uint32_t k = 0; k < L.nslots; k++) m[k] = L.at(L.thread_word(cur, e, 1 + k));
        m[1] = pos;
        matched = true;
        break;
      }
      if (c != RX_NONE && rx_consumes(L, in, c)) {
        for (uint32_t k = 0; k < L.nslots; k++) cap[k] = L.at(L.thread_word(cur, e, 1 + k));
        rx_add(L, cur ^ 1u, nn, seen_n, in.x, t, len, pos + w, cap, fault);
      }
    }
    cur ^= 1u; nc = nn; seen_c = seen_n;
    if (w == 0 || fault) break;
    pos += w;
  }
  return matched;
}

__device__ __forceinline__ void rx_copy(uint8_t *dst, const uint8_t *src, uint32_t n) {
  struct __attribute__((packed, aligned(1))) U64 { uint64_t v; };
  uint32_t i = 0;
  for (; i + 8 <= n; i += 8) reinterpret_cast<U64 *>(dst + i)->v = reinterpret_cast<const U64 *>(src + i)->v;
  for (; i < n; i++) dst[i] = src[i];
}

// Regexp.replaceAll + expand.  WRITE = false: the result's length and whether anything matched; WRITE = true: the bytes.
template <bool WRITE, bool LDSWS>
__global__ void __launch_bounds__(RX_BLOCK) regex_replace_kernel(RxParams p) {
  __shared__ RxInst s_inst[TFGPU_REGEX_MAX_PROG];
  __shared__ uint32_t s_ranges[2 * TFGPU_REGEX_MAX_RANGES];
  for (uint32_t k = threadIdx.x; k < p.ninst; k += blockDim.x) s_inst[k] = p.inst[k];
  for (uint32_t k = threadIdx.x; k < 2 * p.npairs; k += blockDim.x) s_ranges[k] = p.ranges[k];
  __syncthreads();
  RxLane<LDSWS> L;
  L.inst = s_inst; L.ranges = s_ranges;
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  L.ws = p.ws; L.lanes = LDSWS ? blockDim.x : p.lanes; L.lane = LDSWS ? threadIdx.x : lane;
  L.ninst = p.ninst; L.nslots = p.nslots; L.stride = 1 + p.nslots;
  L.stack_base = 2 * p.ninst * L.stride; L.stack_cap = p.stack_cap;
  uint32_t fault = 0, any = 0;
  for (int64_t r = (int64_t)lane; r < p.n; r += (int64_t)p.lanes) {
    const uint32_t a = p.in_off[r], len = p.in_off[r + 1] - a;
    const uint8_t *t = p.in_data + a;
    uint8_t *o = WRITE ? p.out_data + p.out_off[r] : nullptr;
    uint64_t on = 0;  // (64 bits: the host refuses the column before any write pass if a cell, or all of them, would pass 4 GiB)
    if (p.validity && !((p.validity[r >> 3] >> (r & 7)) & 1)) {  // nil: not a string, passed through
      if (WRITE) rx_copy(o, t, len); else p.out_len[r] = len;
      continue;
    }
    if (len > (uint32_t)TFGPU_REGEX_MAX_CELL) {  // refused by the host after the length pass: nothing is searched, nothing written
      fault |= RXF_CELL;
      if (!WRITE) p.out_len[r] = len;
      continue;
    }
    uint64_t budget = ((uint64_t)len + 1) * (p.ninst + 16) + 1024;
    uint32_t last_end = 0, search = 0;
    uint32_t m[RX_MAX_SLOTS];
    while (search <= len) {
      if (!rx_search(L, p.start, t, len, search, m, fault, budget)) break;
      any = 1;
      if (on > 0xFFFFFFFFull) { fault |= RXF_4GIB; break; }
      if (WRITE) rx_copy(o + on, t + last_end, m[0] - last_end);
      on += m[0] - last_end;
      if (m[1] > last_end || m[0] == 0) {  // no copy of the rule for an empty match right behind another match
        for (uint32_t s = 0; s < p.nsegs; s++) {
          const RxSeg sg = p.segs[s];
          if (sg.group < 0) { if (WRITE) rx_copy(o + on, p.lits + sg.off, sg.len); on += sg.len; }
          else {
            const uint32_t b = m[2 * sg.group], e = m[2 * sg.group + 1];
            if (b != RX_NONE && e != RX_NONE) { if (WRITE) rx_copy(o + on, t + b, e - b); on += e - b; }
          }
        }
      }
      last_end = m[1];
      uint32_t w = 0;  // advance past this match, and by one rune at least
      if (search < len) rx_decode(t, search, len, w);
      if (search + w > m[1]) search += w;
      else if (search + 1 > m[1]) search++;
      else search = m[1];
    }
    if (WRITE) rx_copy(o + on, t + last_end, len - last_end);
    on += len - last_end;
    if (on > 0xFFFFFFFFull) fault |= RXF_4GIB;
    if (!WRITE) p.out_len[r] = on > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)on;
  }
  if (!WRITE && (any || fault)) atomicOr(p.flags, any | fault);
  if (WRITE && fault) atomicOr(p.flags, fault);
}

static Buf upload_prog(const RegexProg &rx, RxParams &rp) {
  // one table: instructions, class ranges, rule segments, rule literals
  const size_t ni = rx.inst.size() * sizeof(RxInst), nr = rx.ranges.size() * 4, ns = rx.segs.size() * sizeof(RxSeg), nl = rx.lits.size();
  std::vector<uint8_t> h(ni + nr + ns + nl + 16, 0);
  std::memcpy(h.data(), rx.inst.data(), ni);
  if (nr) std::memcpy(h.data() + ni, rx.ranges.data(), nr);
  if (ns) std::memcpy(h.data() + ni + nr, rx.segs.data(), ns);
  if (nl) std::memcpy(h.data() + ni + nr + ns, rx.lits.data(), nl);
  Buf d = upload_const(h.data(), h.size());
  const uint8_t *b = ptr<uint8_t>(d);
  rp.inst = (const RxInst *)b; rp.ranges = (const uint32_t *)(b + ni); rp.segs = (const RxSeg *)(b + ni + nr); rp.lits = b + ni + nr + ns;
  rp.ninst = (uint32_t)rx.inst.size(); rp.npairs = (uint32_t)rx.ranges.size() / 2; rp.start = rx.start; rp.nslots = (uint32_t)rx.nslots; rp.nsegs = (uint32_t)rx.segs.size();
  return d;
}

std::unique_ptr<tfgpu_dbatch> apply_regex_replace(const tfgpu_plan &p, const tfgpu_dbatch &in) {
  if (!p.tables.match(in.table)) {  // transformer.go:96-99: the loop `continue`s — the item is neither transformed nor an error
    Buf sel = dalloc(4);
    return gather_rows(in, sel, 0);
  }
  if (!in.schema.empty() && in.cols.size() > in.schema.size())
    throw Error(TFGPU_ERR_UNSUPPORTED, "regex_replace_transformer: the batch has more columns than its TableSchema (the stock transformer indexes the schema by the "
                                       "column's position and panics there)");
  // transformer.go:103-112: the DataType of the i-th SCHEMA column decides about the i-th value
  auto rewrites = [&](size_t i) {
    const DColumn &c = in.cols[i];
    if (!p.columns.match(c.name)) return false;
    const int typ = in.schema.empty() ? c.dtype : in.schema[i].second;
    return (typ == TFGPU_T_UTF8 && c.repr == TFGPU_R_STRING) || (typ == TFGPU_T_BYTES && c.repr == TFGPU_R_BYTES);
  };
  {
    std::vector<const DColumn *> need;
    for (size_t i = 0; i < in.cols.size(); i++) if (rewrites(i)) need.push_back(&in.cols[i]);
    materialize(in, &need);
  }
  auto out = std::make_unique<tfgpu_dbatch>(in);
  const int64_t n = in.nrows;
  if (!n) return out;
  hipStream_t st = ctx().stream;
  RxParams rp{};
  Buf prog = upload_prog(*p.rx, rp);
  // working memory per lane: two thread lists of ninst threads (pc + slots) and rx_add's stack.  In LDS when a workgroup of 256, 128 or 64 lanes
  // fits RX_LDS_BUDGET; else in an HBM workspace, and the grid shrinks before that workspace passes 256 MiB.
  rp.stack_cap = 1;
  for (auto &in_ : p.rx->inst) if (in_.op == RX_SPLIT || in_.op == RX_SAVE) rp.stack_cap++;
  const size_t words = (size_t)2 * rp.ninst * (1 + rp.nslots) + 2 * (size_t)rp.stack_cap;
  int block = 0;
  for (int b : {256, 128, 64}) if (!block && words * 4 * (size_t)b <= RX_LDS_BUDGET) block = b;
  const bool lds = block != 0;
  if (!lds) block = RX_BLOCK;
  size_t lanes = std::min<size_t>((size_t)((n + block - 1) / block) * (size_t)block, (size_t)ctx().num_cus * 1024);
  Buf ws;
  if (!lds) {
    lanes = std::min(lanes, std::max<size_t>((size_t)block, ((size_t)256 << 20) / (words * 4) / (size_t)block * (size_t)block));
    ws = dalloc(words * 4 * lanes);
  }
  rp.ws = ptr<uint32_t>(ws); rp.lanes = (uint32_t)lanes; rp.n = n;
  const unsigned grid = (unsigned)(lanes / (size_t)block);
  const size_t shmem = lds ? words * 4 * (size_t)block : 0;
  for (size_t i = 0; i < out->cols.size(); i++) {
    if (!rewrites(i)) continue;
    DColumn &c = out->cols[i];
    rp.in_off = ptr<uint32_t>(c.offsets); rp.in_data = ptr<uint8_t>(c.payload()); rp.validity = ptr<uint8_t>(c.validity);
    Buf off = dalloc((size_t)(n + 1) * 4);
    Buf aux = dalloc_zero(16);  // u64 total, u32 flags
    rp.out_len = ptr<uint32_t>(off); rp.out_off = nullptr; rp.out_data = nullptr;
    rp.flags = ptr<uint32_t>(aux) + 2;
    {
      KernelTimer t("regex_replace_len", n);
      if (lds) regex_replace_kernel<false, true><<<grid, block, shmem, st>>>(rp);
      else regex_replace_kernel<false, false><<<grid, block, shmem, st>>>(rp);
    }
    sum_u32_segments_u64(ptr<uint32_t>(off), n, 1, n, ptr<unsigned long long>(aux));
    const uint32_t *h = d2h_u32(aux->p, 3);
    sync();
    const uint64_t total = (uint64_t)h[0] | (uint64_t)h[1] << 32;
    const uint32_t flags = h[2];
    if (flags & RXF_INTERNAL) throw Error(TFGPU_ERR_DEVICE, "regex_replace_transformer: internal thread-list bound hit");
    if (flags & RXF_CELL)
      throw Error(TFGPU_ERR_UNSUPPORTED, "regex_replace_transformer: column " + c.name + " holds a cell longer than " + std::to_string(TFGPU_REGEX_MAX_CELL) +
                                             " bytes (TFGPU_REGEX_MAX_CELL): one lane walks a cell; keep this batch on the host");
    if (flags & RXF_BUDGET)
      throw Error(TFGPU_ERR_UNSUPPORTED, "regex_replace_transformer: a cell of column " + c.name + " needs more search steps than (length + 1) * (program size + 16) + 1024 — "
                                             "the pattern restarts long searches from many positions (quadratic in Go as well); keep this batch on the host");
    if (!(flags & RXF_MATCHED)) continue;  // nothing matched in this column: its buffers stay
    if ((flags & RXF_4GIB) || total > 0xFFFFFFFFull) throw Error(TFGPU_ERR_UNSUPPORTED, "regex_replace_transformer: column " + c.name + " would pass 4 GiB; split the batch by rows");
    exclusive_scan_u32(ptr<uint32_t>(off), ptr<uint32_t>(off), n, true);
    Buf data = dalloc(std::max<uint64_t>(total, 1));
    rp.out_len = nullptr; rp.out_off = ptr<uint32_t>(off); rp.out_data = ptr<uint8_t>(data);
    {
      KernelTimer t("regex_replace_write", n);
      if (lds) regex_replace_kernel<true, true><<<grid, block, shmem, st>>>(rp);
      else regex_replace_kernel<true, false><<<grid, block, shmem, st>>>(rp);
    }
    DColumn o;
    o.name = c.name; o.dtype = c.dtype; o.repr = c.repr;
    o.offsets = off; o.data = data; o.data_len = total; o.validity = c.validity;
    c = std::move(o);
  }
  return out;
}

}  // namespace tf
