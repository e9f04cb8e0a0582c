// Regular expressions for regexp_like / regexp_matches (round 5): the pattern — a literal of the expression, as for the
// reference's holders, which compile it with RE2 once per expression [regexp_matches_holder.cc / like_holder.cc, as
// recalled] — is compiled HERE, at Make time, into a position automaton (Glushkov: one state per character position of the
// pattern, no epsilon moves) of at most 63 positions, laid out as a table the device function gdv_regex_search walks with
// one 64-bit state set per row.  Assertions consume nothing: they become CONDITIONS on the automaton's edges — conjunctions of
// word boundary / not a word boundary / start of the text / end of the text, at most 8 distinct ones per pattern — evaluated on
// the gap between two bytes:
//     uint64 flags, nullable, predicates[8], first[8], last[8], follow[64][8], match[256]     (GDV_REGEX_TABLE_BYTES = 6352)
// (match[b] = the positions that accept byte b; flags bit 0: every way in asks for the start of the text, bits 8-15: the
// conditions that occur; predicates[c]: what condition c asks).  "Does the text contain a match" is all the two functions ask, so greedy / lazy / leftmost-first
// make no difference and the automaton's answer is RE2's (tests hold it to the RE2 in this image's libarrow).
//
// Syntax taken: literals, '.', classes [a-z0-9_] and [^...] (ASCII members; non-ASCII characters as members of a positive
// class), POSIX classes [[:alpha:]] ... inside brackets, \d \D \w \W \s \S, \t \n \r \f \v \xHH and escaped punctuation,
// groups ( ), (?: ) and (?P<name> ), alternation |, quantifiers * + ? {m} {m,} {m,n} (and their lazy forms), the assertions
// ^ $ \A \z \b \B anywhere, the flags (?i) (ASCII letters in either case — and, as RE2's simple folding has it, U+212A KELVIN
// SIGN with k and U+017F LONG S with s, in positive and negated sets alike) and (?s) ('.' matches a newline) in front of
// everything.  \s / \S are Perl's [\t\n\f\r ] (no vertical tab); [[:space:]] holds it.  '.' and negated classes consume a whole UTF-8 character (a lead byte and its continuation bytes); \b is
// RE2's ASCII word boundary.  Anything else — back-references and look-around (RE2 has neither), flags inside the pattern,
// Unicode classes \p{..}, non-ASCII range ends or negated classes with non-ASCII members, (?i) next to non-ASCII characters,
// more than 7 distinct combinations of assertions, more than 63 positions — is refused with a message, not guessed; so are
// patterns beyond 4096 bytes, 64 levels of nesting or 512 atoms and quantifiers (the tree is walked recursively; patterns come from user SQL).
// Texts that are not valid UTF-8: '.' and negated classes take "a lead byte and whatever continuation bytes follow" as one
// character, which RE2 does not — the two agree on valid UTF-8 only.
//
// regexp_extract(text, 'pattern', index) asks more: WHICH match RE2's unanchored search takes (the leftmost start, then the
// first alternative that leads to a match, greedy quantifiers as long and lazy ones as short as that allows) and where group
// `index` lies in it.  CompileRegexExtract takes the same syntax and limits and lays the same positions out for a walk in
// order of preference (the device function gdv_regex_extract: an ordered list of at most 63 live positions, each with the
// extents of the ONE group asked for; no backtracking, nothing sized by the text):
//     the 6352 bytes above | uint64 flags | uint64 match[256] | uint64 targets[64] | uint16 first[65] (padded to 136 bytes) | uint16 ways[]
// (the table of "is there a match" in front: the row walks that first, with its one 64-bit set, and only a row that holds a
// match walks the ordered lists).
// List p (p < 63: behind position p; 63: into the pattern) = ways[first[p] .. first[p + 1]), most preferred first.  A way is
// target | predicates << 6 | action << 10: the position entered next (63 = the match ends here, which holds its place in the
// order like any other way), the predicates of the gap (1 word boundary, 2 not one, 4 start of the text, 8 end of it — all
// must hold), and what crossing the gap does to the group: 0 nothing, 1 it closes, 2 it opens (a previous iteration closes
// first), 3 it opens and closes on the spot.  targets[p] = the union of list p's targets (a filter); flags bit 0: every way
// in asks for the start of the text.  Groups are numbered by opening parenthesis, (?: ) does not count, (?P<name> ) does; the
// copies a counted repetition makes of a group are the same group (the last iteration is kept).  Refused on top of the list
// above: a repetition without an upper bound whose body can match the empty text — (a*)*, (a|)+, (\b)* — where RE2 stops
// the loop by rules the ordered lists cannot state; tables beyond 32768 bytes.
#pragma once
#include <string>

#include "gdv_types.h"

namespace gdv {

// table = the bytes described above; CodeGenError with the reason otherwise
Status CompileRegex(const std::string& pattern, std::string* table);

// table = the ordered lists for group `group` (0 = the whole match); CodeGenError for what is refused and for a group
// index outside 0 .. the pattern's number of groups
Status CompileRegexExtract(const std::string& pattern, int group, std::string* table);

// to_date's SQL pattern -> one byte per strptime directive, the program gdv_parse_date interprets (gdv_regex.cc)
Status CompileDateFormat(const std::string& pattern, std::string* ops);

}  // namespace gdv
