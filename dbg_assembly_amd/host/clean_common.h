// clean_common.h -- what bin/clean_adapter and bin/clean_lowqual share on top of cli_common.h: the FASTQ record loop of the
// reference (clean_illumina/clean_adapter.cpp:376-387, the same in clean_lowqual.cpp) and a batch of records on its way to the
// device (CLEAN section of include/dbgk.h); and, with DBGK_TEXT=device, the route on which the text of the file never becomes
// strings: parsed, cleaned, compacted, formatted and (with DBGK_GZ=device) deflated where it lies on the device.
#pragma once
#include <unistd.h>
#include <cstdio>
#include <ctime>

#include "cli_common.h"
#include "dbgk_env.h"
#include "text_window.h"

static const uint64_t BatchReads = 1 << 20;   // records per device batch
static const uint64_t BatchBases = 256 << 20; // ... or this many bases, whichever comes first

// a batch of records: heads, reads and qualities as read, and the reads (for clean_lowqual the qualities too) back to back
struct RecordBatch {
	vector<string> heads, reads, quals;
	uint64_t bases = 0;
	size_t size() const { return heads.size(); }
	bool full() const { return size() >= BatchReads || bases >= BatchBases; }
	void clear()
	{
		heads.clear(); reads.clear(); quals.clear();
		bases = 0;
	}
	// the record loop: a line that starts with '@' opens a record and the next three lines are read, separator and quality
	// whatever they hold; every other line outside a record is skipped.  false at the end of the file.
	bool fill(LineReader &in, uint64_t &total_raw_reads, uint64_t &total_raw_bases)
	{
		string head, read, unused, qual;
		while (!full() && in.getline(head)) {
			if (head.empty() || head[0] != '@') continue;
			in.getline(read);
			in.getline(unused);
			in.getline(qual);
			total_raw_reads++;
			total_raw_bases += read.size();
			bases += read.size();
			heads.push_back(head);
			reads.push_back(read);
			quals.push_back(qual);
		}
		return full();
	}
	// every record as four lines, also when read and quality were emptied
	void write(GzWriter &out) const
	{
		string text;
		for (size_t i = 0; i < size(); i++) {
			text += heads[i]; text += '\n';
			text += reads[i]; text += "\n+\n";
			text += quals[i]; text += '\n';
			if (text.size() >= (64u << 20)) {
				out.write(text);
				text.clear();
			}
		}
		out.write(text);
	}
};

// ---- DBGK_TEXT=device -----------------------------------------------------------------------------------------------------------
// Window by window (text_window.h): the decompressed bytes of the input behind what the window before left unconsumed ->
// dbgk_parse_chunk with a quality plane -> the program's cleaner on the
// parser's planes -> dbgk_clean_compact -> dbgk_fmt_records_device with the suffixes the program composes on the host from the
// returned records -> GzWriter::write_device.  The output and the .stat file are byte for byte the host route's; the "reading num"
// lines count a window's records.

struct DeviceTextTotals {
	uint64_t raw_reads = 0, raw_bases = 0; // records, and the bytes of their sequence lines as the text has them
	uint64_t trimmed_reads = 0, trimmed_bases = 0, short_reads = 0, short_bases = 0, clean_reads = 0, clean_bases = 0;
};

// clean(d_bases, d_quals, offsets, lens, n, suffix, suffix_offsets): the program's dbgk_clean_*_device call on the n reads of a
// window (offsets and lens on the host, lens[i] the length of read i after the parser's emptying), and suffix i, the annotation of
// header i, appended to `suffix` with suffix_offsets[i + 1] behind it.  refuse_mismatched: a record whose quality line is not as
// long as its read ends the program (bin/clean_adapter keeps such a line as it is, which the device batch cannot hold).
template <class Clean>
static void clean_text_on_device(const string &in_path, GzWriter &out, dbgk_clean *cleaner, int min_len, bool refuse_mismatched, DeviceTextTotals &T,
                                 Clean clean)
{
	TextWindows in(in_path);
	if (!in.ok()) {
		cerr << "fail to open input file " << in_path << endl;
		return;
	}
	dbgk_parse *parser = nullptr;
	dbgk_fmt *formatter = nullptr;
	int rc = dbgk_parse_create(1, 1, 0, &parser);
	if (rc) die("dbgk_parse_create", rc);
	rc = dbgk_fmt_create(1, 0, 0, &formatter);
	if (rc) die("dbgk_fmt_create", rc);
	vector<uint64_t> offsets, lens, suffix_offsets;
	vector<dbgk_parse_rec> recs;
	string suffix;
	while (in.next()) {
		dbgk_parse_info pi;
		rc = dbgk_parse_chunk(parser, in.text(), in.n_text, in.last ? 1 : 0, &pi);
		if (rc) die("dbgk_parse_chunk", rc);
		const uint64_t n = pi.n_records;
		cerr << "reading num " << n << endl;
		if (refuse_mismatched && pi.mismatched) {
			cerr << pi.mismatched << " record(s) of " << in_path << " have a quality line that is not as long as the read: "
			     << "DBGK_TEXT=device cannot keep such a line, run without it" << endl;
			exit(1);
		}
		if (n) {
			offsets.resize(n + 1);
			recs.resize(n);
			rc = dbgk_parse_results(parser, nullptr, nullptr, offsets.data(), recs.data());
			if (rc) die("dbgk_parse_results", rc);
			const char *d_bases, *d_quals, *d_text;
			const uint64_t *d_offsets;
			const dbgk_parse_rec *d_recs;
			uint64_t n_reads, n_bases, n_bytes;
			rc = dbgk_parse_device(parser, &d_bases, &d_quals, &d_offsets, &n_reads, &n_bases);
			if (rc) die("dbgk_parse_device", rc);
			rc = dbgk_parse_recs_device(parser, &d_recs);
			if (rc) die("dbgk_parse_recs_device", rc);
			rc = dbgk_parse_text_device(parser, &d_text, &n_bytes);
			if (rc) die("dbgk_parse_text_device", rc);
			lens.resize(n);
			for (uint64_t i = 0; i < n; i++) {
				T.raw_bases += recs[i].seq_len; // (counted before a mismatched record is emptied, as the host route does)
				lens[i] = offsets[i + 1] - offsets[i];
			}
			T.raw_reads += n;
			suffix.clear();
			suffix_offsets.assign(1, 0);
			clean(d_bases, d_quals, offsets.data(), lens.data(), n, suffix, suffix_offsets);
			dbgk_clean_compact_info ci;
			rc = dbgk_clean_compact(cleaner, min_len, &ci);
			if (rc) die("dbgk_clean_compact", rc);
			T.trimmed_reads += ci.trimmed_reads, T.trimmed_bases += ci.trimmed_bases;
			T.short_reads += ci.short_reads, T.short_bases += ci.short_bases;
			T.clean_reads += ci.clean_reads, T.clean_bases += ci.clean_bases;
			const char *c_bases, *c_quals;
			const uint64_t *c_offsets;
			rc = dbgk_clean_compact_device(cleaner, &c_bases, &c_quals, &c_offsets, &n_reads, &n_bases);
			if (rc) die("dbgk_clean_compact_device", rc);
			dbgk_fmt_info fi;
			rc = dbgk_fmt_records_device(formatter, d_text, n_bytes, d_recs, c_bases, c_quals, c_offsets, n, suffix.data(), suffix_offsets.data(), &fi);
			if (rc) die("dbgk_fmt_records_device", rc);
			out.write_device(formatter);
		}
		in.keep_from(pi.consumed);
	}
	dbgk_fmt_destroy(formatter);
	dbgk_parse_destroy(parser);
}
