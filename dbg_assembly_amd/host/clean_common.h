// clean_common.h -- what bin/clean_adapter and bin/clean_lowqual share: gzip line input and output, the FASTQ record loop of the
// reference (clean_illumina/clean_adapter.cpp:376-387, the same in clean_lowqual.cpp) and a batch of records on its way to the
// device (CLEAN section of include/dbgk.h).
#pragma once
#include <unistd.h>
#include <zlib.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "dbgk.h"

using namespace std;

static const uint64_t BatchReads = 1 << 20;   // records per device batch
static const uint64_t BatchBases = 256 << 20; // ... or this many bases, whichever comes first

static void die(const char *what, int rc)
{
	cerr << what << " failed: " << dbgk_strerror(rc);
	if (rc == DBGK_ERR_HIP) cerr << " [" << dbgk_last_error() << "]";
	cerr << endl;
	exit(1);
}

// getline over a plain or gzip file (what igzstream + getline read)
struct LineReader {
	gzFile f = nullptr;
	vector<char> buf = vector<char>(1 << 20);
	size_t pos = 0, len = 0;
	bool eof = false;
	explicit LineReader(const string &path)
	{
		f = gzopen(path.c_str(), "rb");
		if (!f) cerr << "fail to open input file " << path << endl;
	}
	~LineReader() { if (f) gzclose(f); }
	bool getline(string &s)
	{
		s.clear();
		bool any = false;
		for (;;) {
			if (pos == len) {
				if (eof || !f) return any;
				const int n = gzread(f, buf.data(), (unsigned)buf.size());
				if (n <= 0) { eof = true; return any; }
				pos = 0;
				len = (size_t)n;
			}
			any = true;
			const char *b = buf.data() + pos;
			const char *nl = (const char *)memchr(b, '\n', len - pos);
			if (nl) {
				s.append(b, nl - b);
				pos += (nl - b) + 1;
				return true;
			}
			s.append(b, len - pos);
			pos = len;
		}
	}
};

// what ogzstream writes
struct GzWriter {
	gzFile f = nullptr;
	explicit GzWriter(const string &path)
	{
		f = gzopen(path.c_str(), "wb");
		if (!f) cerr << "fail to open output file " << path << endl;
	}
	~GzWriter() { if (f) gzclose(f); }
	void write(const string &s)
	{
		if (f && !s.empty()) gzwrite(f, s.data(), (unsigned)s.size());
	}
};

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

static void concat(const vector<string> &v, string &bases, vector<uint64_t> &offsets)
{
	bases.clear();
	offsets.assign(1, 0);
	for (const string &s : v) {
		bases += s;
		offsets.push_back(bases.size());
	}
}
