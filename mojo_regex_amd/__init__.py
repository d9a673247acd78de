"""mojo_regex_amd -- MI355X-native batch regex matcher.

Python host layer above the C ABI (include/mrx.h, libmrx_hip.so).  It mirrors
the reference's public interface for the matching hot path -- same names and
argument meaning, a *batch* of texts instead of one text:

    reference (src/regex/matcher.mojo)            here
    ------------------------------------------    ------------------------------
    compile_regex(pattern)            :1292       compile_regex(pattern)
    CompiledRegex.match_first(text)   :1049       CompiledRegex.match_first(texts)
    CompiledRegex.match_next(text)    :1064       CompiledRegex.match_next(texts)
    CompiledRegex.match_all(text)     :1078       CompiledRegex.match_all(texts)
    CompiledRegex.is_match(text)      :1104       CompiledRegex.is_match(texts)
    CompiledRegex.sub(repl, text)     :1118       CompiledRegex.sub(repl, texts)
    CompiledRegex.get_stats()         :1139       CompiledRegex.get_stats()
    match_first / search / findall    :1325-1415  match_first / search / findall
    (none: sub()'s loop with groups)  :1679-1854  captures_all / CompiledRegex.captures_all
    split / sub                       :1357,1857  split / sub
    clear_regex_cache()               :1318       clear_regex_cache()
    (none: one pattern per call)                  PatternSet / compile_set(patterns): k at once
    (none: k sub() calls in a row)                PatternSet.sub(repls, texts): k patterns' hits, one call
    CompiledRegex.test(text), per text :1091      filter_texts / CompiledRegex.filter / PatternSet.filter:
                                                  the matching texts as a new packed batch
    Match.get_match_text(), per match             findall_texts / CompiledRegex.extract / split_batch /
                                                  PatternSet.extract / DeviceBatch.gather_spans: the matched
                                                  bytes as a new packed batch
    Match groups into a template, per match       expand / CompiledRegex.expand / DeviceBatch.expand_spans:
                                                  one templated record per match as a new packed batch
    (none: a Dict[String, Int] on the host)       distinct / value_counts / DeviceBatch.distinct /
                                                  CompiledRegex.value_counts: the unique texts and their counts
    (none: `x in dict` / dict[x] on the host)     Dictionary / build_dictionary / lookup: the index of every
                                                  text in a fixed set of entries, isin and semi- / anti-join
    (none: sorted(...) on the host)               sort_texts / DeviceBatch.argsort / take / sort, and sort= /
                                                  top= of value_counts and distinct: the bytewise order of a
                                                  batch's texts, and the texts at given indices as a new batch
    (none: bisect / startswith on the host)       SortedIndex / build_sorted_index / searchsorted: bisect,
                                                  the entries that begin with a text and the longest entry
                                                  that is a prefix of it, against sorted entries
    (none: int(m.get_match_text()) per match)     numbers / parse_numbers / CompiledRegex.numbers /
                                                  DeviceBatch.parse / parse_spans: pieces as int64 / float64
    (none: "%s %d\\n" % row on the host)          format_records / format_numbers / format_records_async:
                                                  text and number columns as packed records, the report's bytes
    (none: one alternation of literals per call)  Keywords / build_keywords / keywords_filter: which of
                                                  thousands of literals occur inside each text, one pass
    (none: one re.sub per literal on the host)    Keywords.sub / subn / leftmost / keywords_sub: the
                                                  leftmost-longest matches of a keyword set, and every text
                                                  with them replaced, per entry or by one replacement
    (none: text.split("\\n") on the host)         lines_of / DeviceBatch.from_lines / lines / lines_async: a
                                                  buffer's bytes as the packed batch of its lines
    (none: text.split()[k] on the host)           fields_of / DeviceBatch.fields / fields_async / cut: the
                                                  columns of every text as span rows, no pattern involved
    (none: csv.reader on the host)                csv_of / csv_columns / DeviceBatch.fields(quote=): quoted
                                                  CSV cells and quoted log-line columns
    (none: text.lower() / .translate() / .strip() translate_texts / strip_texts / DeviceBatch.translate / lower /
     on the host)                                 upper / strip and their _async forms: tr, case folding and
                                                  trimming of every text, no pattern involved

All matching runs in the HIP kernels of libmrx_hip.so.  There is no CPU
fallback: if the library is missing or no GPU is usable, calls raise.
(The directory is named mojo_regex_amd because Python cannot import a package
whose name contains '-'.)
"""
from .api import (  # noqa: F401
    CompiledRegex,
    DeviceBatch,
    Dictionary,
    Keywords,
    MrxError,
    PatternSet,
    RegexSyntaxError,
    SortedIndex,
    UnsupportedPattern,
    build_dictionary,
    build_keywords,
    build_sorted_index,
    captures_all,
    clear_regex_cache,
    compile_regex,
    compile_set,
    csv_columns,
    csv_of,
    distinct,
    expand,
    fields_of,
    filter_texts,
    findall,
    findall_texts,
    format_numbers,
    format_records,
    format_records_async,
    keywords_filter,
    keywords_sub,
    library_path,
    lines_of,
    load_library,
    lookup,
    match_first,
    numbers,
    pack_texts,
    parse_numbers,
    search,
    searchsorted,
    sort_texts,
    split,
    strip_texts,
    sub,
    translate_texts,
    value_counts,
)
