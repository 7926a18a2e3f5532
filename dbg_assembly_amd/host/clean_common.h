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
// Window by window: the decompressed bytes of the input (zlib's gzread: plain and ordinary gzip alike; DBGK_GUNZIP is not looked
// at) behind what the window before left unconsumed -> dbgk_parse_chunk with a quality plane -> the program's cleaner on the
// parser's planes -> dbgk_clean_compact -> dbgk_fmt_records_device with the suffixes the program composes on the host from the
// returned records -> GzWriter::write_device.  The output and the .stat file are byte for byte the host route's; the "reading num"
// lines count a window's records.

static bool text_on_device()
{
	const char *e = getenv("DBGK_TEXT");
	return e && strcmp(e, "device") == 0;
}

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
	size_t window = (size_t)256 << 20;
	if (const char *h = dbgk_hook("text_window")) // (tests: windows that end inside records of small files; every value gives the same files)
		if (atoll(h) > 0) window = (size_t)atoll(h);
	gzFile in = gzopen(in_path.c_str(), "rb");
	if (!in) {
		cerr << "fail to open input file " << in_path << endl;
		return;
	}
	dbgk_parse *parser = nullptr;
	dbgk_fmt *formatter = nullptr;
	int rc = dbgk_parse_create(1, 1, 0, &parser);
	if (rc) die("dbgk_parse_create", rc);
	rc = dbgk_fmt_create(1, 0, 0, &formatter);
	if (rc) die("dbgk_fmt_create", rc);
	vector<char> chunk;
	vector<uint64_t> offsets, lens, suffix_offsets;
	vector<dbgk_parse_rec> recs;
	string suffix;
	size_t have = 0;
	for (bool last = false; !last;) {
		if (have + window >= ((size_t)1 << 31)) {
			cerr << "a record of " << in_path << " does not end within 2 GiB of text: DBGK_TEXT=device cannot read this file" << endl;
			exit(1);
		}
		chunk.resize(have + window);
		size_t got = 0;
		while (got < window) {
			const int r = gzread(in, chunk.data() + have + got, (unsigned)min<size_t>(window - got, 1u << 30));
			if (r < 0) {
				cerr << "fail to read input file " << in_path << endl;
				exit(1);
			}
			if (r == 0) {
				last = true;
				break;
			}
			got += (size_t)r;
		}
		const size_t n_text = have + got;
		dbgk_parse_info pi;
		rc = dbgk_parse_chunk(parser, chunk.data(), n_text, last ? 1 : 0, &pi);
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
		// what the window left unconsumed goes in front of the next one; a window without a whole record only makes the text longer
		have = last ? 0 : n_text - (size_t)pi.consumed;
		if (have && pi.consumed) memmove(chunk.data(), chunk.data() + pi.consumed, have);
	}
	gzclose(in);
	dbgk_fmt_destroy(formatter);
	dbgk_parse_destroy(parser);
}
